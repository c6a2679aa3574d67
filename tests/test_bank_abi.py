"""fheram_bank_create / RamBank: the argument checks that run before a device is asked for (no compute calls: this runs on the
CPU-only build box).  Order (include/fheram.h): null pointers, n_members outside [1, FHERAM_BANK_MAX] and n_members * word_size > 64
-> INVALID_ARG; the parameter checks of fheram_ctx_create_cfg, same codes and messages; only then "no HIP device"."""
import ctypes as C
import subprocess
import sys

import pytest

from _pkg import load_package

ST_INVALID_ARG, ST_UNSUPPORTED, ST_DEVICE = 1, 5, 7


def _create(cp, n_members, out=None):
    L = load_package().library()
    out = C.c_void_p() if out is None else out
    rc = L.fheram_bank_create(C.byref(cp), 0, n_members, None, C.byref(out))
    return rc, L.fheram_bank_last_error(None).decode(), out


def _default_params():
    pkg = load_package()
    cp = pkg.api._CParams()
    assert pkg.library().fheram_params_default(C.byref(cp)) == 0
    return cp


def test_bank_max_matches_the_header():
    import os
    import re
    pkg = load_package()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"#define\s+FHERAM_BANK_MAX\s+(\d+)", open(os.path.join(root, "include", "fheram.h")).read())
    assert m and int(m.group(1)) == pkg.api.BANK_MAX == 8


@pytest.mark.parametrize("n_members", [0, 9, -1])
def test_member_count_outside_the_limit_is_refused(n_members):
    rc, msg, out = _create(_default_params(), n_members)
    assert rc == ST_INVALID_ARG and "n_members" in msg and out.value is None, (rc, msg)


def test_more_than_64_ciphertexts_is_refused():
    cp = _default_params()
    cp.word_size = 16
    rc, msg, out = _create(cp, 8)
    assert rc == ST_INVALID_ARG and "64" in msg and out.value is None, (rc, msg)


def test_null_pointers_are_refused():
    L = load_package().library()
    out = C.c_void_p()
    assert L.fheram_bank_create(None, 0, 2, None, C.byref(out)) == ST_INVALID_ARG
    assert L.fheram_bank_create(C.byref(_default_params()), 0, 2, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_last_error(None)
    # a null bank is refused by every entry point, and harmless to destroy
    assert L.fheram_bank_size(None) == 0 and L.fheram_bank_ram_state(None, 0) == 0
    assert L.fheram_bank_sync(None) == ST_INVALID_ARG
    assert L.fheram_bank_read(None, 0, 1, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_write(None, 0, 1, None, None) == ST_INVALID_ARG
    L.fheram_bank_destroy(None)


def test_parameter_checks_are_those_of_a_context():
    L = load_package().library()
    cp = _default_params()
    cp.log_n = 11
    out = C.c_void_p()
    assert L.fheram_ctx_create(C.byref(cp), 0, C.byref(out)) == ST_UNSUPPORTED
    want = L.fheram_last_error(None).decode()
    rc, msg, _ = _create(cp, 2)
    assert rc == ST_UNSUPPORTED and msg == want and "LOG_N=12" in msg, (rc, msg)
    cp = _default_params()
    cp.decomp_n[0] = 4
    assert L.fheram_ctx_create(C.byref(cp), 0, C.byref(out)) == ST_INVALID_ARG
    want = L.fheram_last_error(None).decode()
    rc, msg, _ = _create(cp, 2)
    assert rc == ST_INVALID_ARG and msg == want, (rc, msg)
    # the member count is checked first
    cp.log_n = 11
    rc, msg, _ = _create(cp, 9)
    assert rc == ST_INVALID_ARG and "n_members" in msg


def _gpu_present():
    # torch is asked in a fresh process (see test_library_abi.py)
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True, timeout=300)
    return r.stdout.strip().endswith("True")


def test_no_gpu_means_loud_failure_not_a_cpu_fallback():
    if _gpu_present():
        pytest.skip("GPU present")
    rc, msg, out = _create(_default_params(), 2)
    assert rc == ST_DEVICE and "no CPU path" in msg and out.value is None, (rc, msg)
    pkg = load_package()
    with pytest.raises(pkg.FheRamError) as e:
        pkg.RamBank(pkg.Parameters.new(), 2)
    assert e.value.code == ST_DEVICE and "no CPU path" in e.value.msg


def test_rambank_refuses_the_same_calls():
    pkg = load_package()
    for n in (0, 9):
        with pytest.raises(pkg.FheRamError) as e:
            pkg.RamBank(pkg.Parameters.new(), n)
        assert e.value.code == ST_INVALID_ARG and "n_members" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:
        pkg.RamBank(pkg.Parameters(word_size=16), 8)
    assert e.value.code == ST_INVALID_ARG and "64" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:
        pkg.RamBank(pkg.Parameters.new(), 2, config={"no_such_switch": 1})
    assert e.value.code == ST_INVALID_ARG
    with pytest.raises(pkg.FheRamError) as e:     # a limb count the kernels are not built for: the context's own refusal
        pkg.RamBank(pkg.Parameters(k_glwe_ct=68), 2)
    assert e.value.code == ST_UNSUPPORTED and "LOG_N=12" in e.value.msg
