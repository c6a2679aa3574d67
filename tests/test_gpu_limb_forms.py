"""Directed device test of the limb arithmetic (csrc/limb_forms.hpp): the scalar forms the chain kernels call — the limb walk,
rsh(1), the closed-form normalisation (take_digit, cmod17 / cmod34, window51, fold_limb_1, the hand-over Y = ceil(A / 2), the
write post-step, the pair forms) and the CMux carries — run on the device by fheram_selftest_limb_forms, one coefficient per
thread, compiled with the library's own flags, and compared with exact integers (tests/_limb_reference.py) and, bit for bit,
with the host build of the same text (tests/limb_forms_host.cpp).  The inputs are the ones the end-to-end tests practically
never produce: rounding ties in one and in several limbs at once, V on the edges of the digit window, the largest |V| the
documented bounds allow, a second quotient of +-2^16.  Each case is one launch; integers only: no tolerance."""
import numpy as np
import pytest

from _pkg import load_package

import _limb_host as H
import _limb_reference as R
from test_limb_forms import check_closed_is_the_limb_walk, check_digit_forms_agree, check_form, check_rsh1_is_the_digits_of_y

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    pkg = load_package()
    ram = pkg.Ram.new_from_ram_params(4, [3, 3, 3, 3], 4096)
    return ram.selftest_limb_forms


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return H.build_shared(tmp_path_factory.mktemp("limb_forms"))


@pytest.mark.parametrize("name", list(R.FORMS))
def test_form_equals_exact_integers_and_the_host_build(device, host, name):
    form = R.FORMS[name]
    out = check_form(device, form)
    assert out.tobytes() == host(form, R.cases(form)[0]).tobytes()      # bit for bit, the signs of zeros included


def test_digits3_and_wrapped_agree(device):
    check_digit_forms_agree(device)


def test_rsh1_is_the_wrapped_digits_of_y(device):
    check_rsh1_is_the_digits_of_y(device)


@pytest.mark.parametrize("name", ["CLOSED4", "CLOSED5"])
def test_closed_form_is_the_limb_walk(device, name):
    check_closed_is_the_limb_walk(device, R.FORMS[name])


def test_bad_arguments_are_refused(device):
    pkg = load_package()
    with pytest.raises(pkg.FheRamError):
        device(len(R.FORMS), np.zeros((1, R.LF_IN)))
    with pytest.raises(pkg.FheRamError):
        device(0, np.zeros(((1 << 20) + 1, R.LF_IN)))
