"""The limb forms the kernels call (fhe-ram_amd/csrc/limb_forms.hpp: the limb walk, rsh(1), the closed-form normalisation of
the chain kernels, the CMux carries) against exact integers — on the CPU, through a host build of the same text
(tests/limb_forms_host.cpp over csrc/limb_forms_eval.hpp, -ffp-contract=off).  tests/test_gpu_limb_forms.py runs the same
inputs through the device build.  Inputs, reference and the asserted preconditions: tests/_limb_reference.py.  All comparisons
are on integers: no tolerance."""
import subprocess

import numpy as np
import pytest

import _limb_host as H
import _limb_reference as R

pytestmark = pytest.mark.skipif(not H.have_compiler(), reason="no g++")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return H.build_shared(tmp_path_factory.mktemp("limb_forms"))


def check_form(run, form):
    """every output of `form` equals the reference, as integers"""
    inp, exp, n_out = R.cases(form)
    out = run(form, inp)
    assert out.shape == exp.shape
    assert np.array_equal(out, np.rint(out)) and np.all(np.abs(out) < 2.0 ** 53)
    got = out.astype(np.int64)
    bad = np.nonzero((got[:, :n_out] != exp[:, :n_out]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), inp[bad[:3]].astype(np.int64).tolist(), got[bad[:3]].tolist(), exp[bad[:3]].tolist())
    assert not got[:, n_out:].any()          # what a form does not produce stays untouched
    return out


def check_digit_forms_agree(run):
    """DIGITS3 and DIGITS3_WRAPPED: the two low digits agree, the top digit agrees modulo 2^17; digit3_r is digit r of DIGITS3"""
    inp, _, _ = R.cases(R.DIGITS3)
    q = run(R.DIGITS3, inp).astype(np.int64)
    w = run(R.DIGITS3_WRAPPED, inp).astype(np.int64)
    assert np.array_equal(q[:, 1:3], w[:, 1:3])
    assert not ((q[:, 0] - w[:, 0]) % (1 << 17)).any()
    assert np.all((w[:, 0] >= -(1 << 16)) & (w[:, 0] < (1 << 16)))
    assert np.any(q[:, 0] == (1 << 16)) and np.any(q[:, 0] == -(1 << 16))      # the quotient +-2^16 does occur as the top digit
    assert np.array_equal(q[:, 0:3], q[:, 3:6])


def check_rsh1_is_the_digits_of_y(run):
    """RSH1<3> equals the wrapped digits of Y_OF, digit for digit — with the rotation's sign: rsh1 of the negated limbs"""
    x, _, _ = R.cases(R.RSH1_3)
    for neg in (0, 1):
        yin = x.copy()
        yin[:, 3] = neg
        y = run(R.Y_OF, yin)
        din = np.zeros_like(x)
        din[:, 0] = y[:, 0]
        d = run(R.DIGITS3_WRAPPED, din)
        xin = x.copy()
        xin[:, :3] *= (1 - 2 * neg)
        assert np.array_equal(d[:, :3], run(R.RSH1_3, xin)[:, :3])


def check_closed_is_the_limb_walk(run, form):
    """CLOSED<SK> equals the limb walk of acc_j + x_j (x: rsh1's limbs, whose integer is the start value): here with the walk's
    inputs built from the device's own RSH1 and NORM outputs where SK limbs fit a NORM form (SK = 4)"""
    inp, exp, _ = R.cases(form)
    sk = 4 if form == R.CLOSED4 else 5
    out = run(form, inp).astype(np.int64)
    lim = inp[:, 1:1 + sk].astype(np.int64)
    lim[:, :3] += R.digits51(inp[:, 0].astype(np.int64))
    assert np.array_equal(out[:, 1:4], R.walk(lim, 3))
    assert np.array_equal(out[:, 0], R.whole(out[:, 1:4]))
    assert np.array_equal(out[:, 4], R.ceil_half(out[:, 0]))
    if sk == 4:
        w = np.zeros_like(inp)
        w[:, :4] = lim.astype(np.float64)
        assert np.array_equal(run(R.NORM4, w)[:, :3].astype(np.int64), out[:, 1:4])


@pytest.mark.parametrize("name", list(R.FORMS))
def test_form_equals_exact_integers(host, name):
    check_form(host, R.FORMS[name])


def test_digits3_and_wrapped_agree(host):
    check_digit_forms_agree(host)


def test_rsh1_is_the_wrapped_digits_of_y(host):
    check_rsh1_is_the_digits_of_y(host)


@pytest.mark.parametrize("name", ["CLOSED4", "CLOSED5"])
def test_closed_form_is_the_limb_walk(host, name):
    check_closed_is_the_limb_walk(host, R.FORMS[name])


def test_grids_hold_the_sharp_inputs():
    """the directed inputs are there: V within +-2 of the window's edges, the largest |V|, ties in every limb at once"""
    for form, sk in ((R.CLOSED4, 4), (R.CLOSED5, 5)):
        inp, _, _ = R.cases(form)
        x = inp.astype(np.int64)
        v = R.closed_v(x[:, 0], x[:, 1:1 + sk])
        for t in (-R.C, R.P51 - R.C, -R.C - R.P51):
            for d in (-2, -1, 0, 1, 2):
                assert np.any(v == t + d)
        assert np.abs(v).max() > 3 * (1 << 50)
        lim = x[:, 1:1 + sk].copy()
        lim[:, :3] += R.digits51(x[:, 0])
        c = np.zeros(len(x), dtype=np.int64)
        ties = np.ones(len(x), dtype=bool)
        for j in range(sk - 1, 0, -1):
            ties &= ((lim[:, j] + c) % (1 << 17)) == (1 << 16)
            c = R.carry(lim[:, j] + c)
        assert ties.sum() >= 100


def test_sanitized_standalone_run(tmp_path):
    """the same text as a stand-alone program under -fsanitize=undefined,address (never loaded into Python): the whole edge grid,
    once; its digest equals the one of the ctypes build's outputs"""
    grid = tmp_path / "grid.bin"
    grid.write_bytes(R.grid_file_bytes())
    exe, sanitized = H.build_program(tmp_path, sanitize=True)
    if not sanitized:
        print("the sanitizers' runtime is not on this machine: the stand-alone program ran without them")
    r = subprocess.run([exe, str(grid)], capture_output=True, text=True, timeout=600)
    grid.unlink()
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    run = H.build_shared(tmp_path)
    dg, at = 0, 0
    for form in range(len(R.FORMS)):
        d, at = R.digest(run(form, R.cases(form, 256)[0]), at)
        dg = (dg + d) % (1 << 64)
    assert r.stdout.split() == ["forms", str(len(R.FORMS)), "coefficients", str(at // R.LF_OUT), "wrong", "0", "digest", "%016x" % dg]
