"""fheram_bank_read_prepare_write_list / fheram_bank_write_list: what can be checked without a device (no compute calls: this runs on the
CPU-only build box).  The header declares the two calls, the library exports them with the declared signatures, the three mirrors exist,
a null bank — with whatever else is null — is refused without a crash, and the header no longer says that there is no list form."""
import ctypes as C
import os
import re

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_INVALID_ARG = 1
I64P = C.POINTER(C.c_int64)
CALLS = ("fheram_bank_read_prepare_write_list", "fheram_bank_write_list")


def _header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


def _decl(name):
    """the declaration of `name` in the header, white space squeezed"""
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
    assert m, name + " is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_both_calls():
    assert _decl("fheram_bank_read_prepare_write_list") == ["fheram_bank* bank", "const int* members", "const fheram_addr* const* addrs", "int n", "int64_t* out"]
    assert _decl("fheram_bank_write_list") == ["fheram_bank* bank", "const int* members", "const fheram_addr* const* addrs", "int n", "const int64_t* w"]


def test_the_allocation_self_test_is_declared_and_refuses_a_null_bank():
    assert _decl("fheram_bank_selftest_fail_list_alloc") == ["fheram_bank* bank", "int nth"]
    L = load_package().library()
    assert L.fheram_bank_selftest_fail_list_alloc(None, 1) == ST_INVALID_ARG


def test_header_no_longer_denies_a_list_form():
    text = re.sub(r"\s+", " ", _header())
    assert "no list form" not in text
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert "There is no list form" not in re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read()), doc


def test_library_exports_both_calls_with_the_declared_signatures():
    pkg = load_package()
    L = pkg.library()
    raw = C.CDLL(pkg.library_path())   # the symbols themselves, not the package's bindings
    bound = pkg.api.exported_symbols()
    for name in CALLS:
        assert getattr(raw, name)
        assert name in bound
        f = getattr(L, name)             # (bank, const int*, const fheram_addr* const*, int, [const] int64_t*) -> int
        assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, I64P], name


def test_null_arguments_are_refused_without_a_crash():
    L = load_package().library()
    members = (C.c_int * 2)(1, 0)
    addrs = (C.c_void_p * 2)(None, None)
    buf = (C.c_int64 * 4)()
    for name in CALLS:
        f = getattr(L, name)
        assert f(None, members, addrs, 2, buf) == ST_INVALID_ARG, name
        assert f(None, None, addrs, 2, buf) == ST_INVALID_ARG, name
        assert f(None, members, None, 2, buf) == ST_INVALID_ARG, name
        assert f(None, members, addrs, 2, None) == ST_INVALID_ARG, name
        assert f(None, None, None, 0, None) == ST_INVALID_ARG, name


def test_the_mirrors_exist():
    pkg = load_package()
    assert callable(pkg.RamBank.read_prepare_write_list) and callable(pkg.RamBank.write_list)
    hpp = open(os.path.join(ROOT, "fhe-ram_amd", "host", "fheram.hpp")).read()
    bank = hpp[hpp.index("class Bank {"):]
    assert re.search(r"\bread_prepare_write_list\s*\(", bank) and "fheram_bank_read_prepare_write_list(" in bank
    assert re.search(r"\bwrite_list\s*\(", bank) and "fheram_bank_write_list(" in bank
    check = open(os.path.join(ROOT, "fhe-ram_amd", "host", "host_check.cpp")).read()
    assert "read_prepare_write_list(" in check and "write_list(" in check
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn fheram_bank_read_prepare_write_list(" in rust and "fn fheram_bank_write_list(" in rust
    assert "fn read_prepare_write_list(" in rust and "fn write_list(" in rust
