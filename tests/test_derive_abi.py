"""fheram_address_alloc / fheram_address_derive and their bank forms (include/fheram.h): the symbols, their signatures as api.py binds
them, and the argument checks that need no device (this runs on the CPU-only build box)."""
import ctypes as C
import os
import re

import pytest

from _pkg import load_package

ST_INVALID_ARG = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VP, VPP, I64P = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)
WANT = {
    "fheram_address_alloc": (C.c_int, [VP, VPP]),
    "fheram_address_derive": (C.c_int, [VP, VPP, C.c_int, C.c_int, VPP]),
    "fheram_bank_fheuint_create": (C.c_int, [VP, I64P, C.c_int, VPP]),
    "fheram_bank_address_alloc": (C.c_int, [VP, VPP]),
    "fheram_bank_address_derive": (C.c_int, [VP, VPP, C.c_int, C.c_int, VPP]),
}
HEADER = {
    "fheram_address_alloc": r"int fheram_address_alloc\(fheram_ctx\* ctx, fheram_addr\*\* out\);",
    "fheram_address_derive": r"int fheram_address_derive\(fheram_ctx\* ctx, const fheram_fheuint\* const\* fus, int n, int sign, fheram_addr\* const\* addrs\);",
    "fheram_bank_fheuint_create": r"int fheram_bank_fheuint_create\(fheram_bank\* bank, const int64_t\* bits, int n_bits, fheram_fheuint\*\* out\);",
    "fheram_bank_address_alloc": r"int fheram_bank_address_alloc\(fheram_bank\* bank, fheram_addr\*\* out\);",
    "fheram_bank_address_derive": r"int fheram_bank_address_derive\(fheram_bank\* bank, const fheram_fheuint\* const\* fus, int n, int sign, fheram_addr\* const\* addrs\);",
}


def _header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


def test_derive_max_is_mirrored():
    pkg = load_package()
    m = re.search(r"#define\s+FHERAM_DERIVE_MAX\s+(\d+)", _header())
    assert m and int(m.group(1)) == pkg.api.DERIVE_MAX == 8


@pytest.mark.parametrize("name", sorted(WANT))
def test_symbol_resolves_with_the_declared_signature(name):
    pkg = load_package()
    L = pkg.library()
    f = getattr(L, name)                      # exported by the library
    res, args = WANT[name]
    assert f.restype is res and list(f.argtypes) == args, (name, f.restype, f.argtypes)
    assert name in pkg.api.exported_symbols()
    assert re.search(HEADER[name], _header()), name   # declared in the header with the issue's signature


def test_null_context_or_bank_is_refused():
    L = load_package().library()
    out = C.c_void_p()
    one = (C.c_void_p * 1)(None)
    bits = (C.c_int64 * 4)()
    assert L.fheram_address_alloc(None, C.byref(out)) == ST_INVALID_ARG and out.value is None
    assert L.fheram_address_derive(None, one, 1, 0, one) == ST_INVALID_ARG
    assert L.fheram_bank_fheuint_create(None, bits, 1, C.byref(out)) == ST_INVALID_ARG and out.value is None
    assert L.fheram_bank_address_alloc(None, C.byref(out)) == ST_INVALID_ARG and out.value is None
    assert L.fheram_bank_address_derive(None, one, 1, 0, one) == ST_INVALID_ARG


def test_null_out_and_null_lists_do_not_crash():
    """A box without a GPU can name no live context or bank, so all this shows is that null `out` / null lists beside a null owner are
    refused without being dereferenced.  A null `out` with a LIVE handle is refused in tests/test_gpu_derive.py (test_refusals_change_nothing)."""
    L = load_package().library()
    bits = (C.c_int64 * 4)()
    assert L.fheram_address_alloc(None, None) == ST_INVALID_ARG
    assert L.fheram_bank_address_alloc(None, None) == ST_INVALID_ARG
    assert L.fheram_bank_fheuint_create(None, bits, 1, None) == ST_INVALID_ARG
    assert L.fheram_address_derive(None, None, 1, 0, None) == ST_INVALID_ARG
    assert L.fheram_bank_address_derive(None, None, 1, 0, None) == ST_INVALID_ARG


def test_python_mirrors_exist():
    pkg = load_package()
    assert callable(pkg.Address.alloc) and callable(pkg.Ram.derive_addresses) and callable(pkg.RamBank.derive_addresses)
    with pytest.raises(pkg.FheRamError) as e:     # the list length is checked before any handle is touched (owner: never looked at)
        pkg.api._derive_addresses(None, None, [], None, False)
    assert e.value.code == ST_INVALID_ARG and "DERIVE_MAX" in e.value.msg
