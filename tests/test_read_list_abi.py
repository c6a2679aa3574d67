"""fheram_bank_read_list / fheram_bank_read_list_result: what can be checked without a device (no compute calls: this runs on the
CPU-only build box).  The header declares the two calls and FHERAM_READ_LIST_MAX, the library exports them with the declared
signatures, the three mirrors exist, and a null bank — with whatever else is null — is refused without a crash."""
import ctypes as C
import os
import re

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_INVALID_ARG = 1
I64P = C.POINTER(C.c_int64)


def _header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


def _decl(name):
    """the declaration of `name` in the header, white space squeezed"""
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
    assert m, name + " is not declared"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_declares_both_calls_and_the_limit():
    assert _decl("fheram_bank_read_list") == ["fheram_bank* bank", "const int* members", "const fheram_addr* const* addrs", "int n", "int64_t* out"]
    assert _decl("fheram_bank_read_list_result") == ["fheram_bank* bank", "int first", "int n", "int64_t* out"]
    m = re.search(r"#define\s+FHERAM_READ_LIST_MAX\s+(\d+)", _header())
    assert m and int(m.group(1)) == 8


def test_python_constant_mirrors_the_header():
    pkg = load_package()
    m = re.search(r"#define\s+FHERAM_READ_LIST_MAX\s+(\d+)", _header())
    assert m and int(m.group(1)) == pkg.api.READ_LIST_MAX


def test_library_exports_both_calls_with_the_declared_signatures():
    pkg = load_package()
    L = pkg.library()
    raw = C.CDLL(pkg.library_path())   # the symbols themselves, not the package's bindings
    assert raw.fheram_bank_read_list and raw.fheram_bank_read_list_result
    bound = pkg.api.exported_symbols()
    assert "fheram_bank_read_list" in bound and "fheram_bank_read_list_result" in bound
    f = L.fheram_bank_read_list        # (bank, const int*, const fheram_addr* const*, int, int64_t*) -> int
    assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, I64P]
    g = L.fheram_bank_read_list_result   # (bank, int, int, int64_t*) -> int
    assert g.restype is C.c_int and list(g.argtypes) == [C.c_void_p, C.c_int, C.c_int, I64P]


def test_null_arguments_are_refused_without_a_crash():
    L = load_package().library()
    members = (C.c_int * 2)(0, 0)
    addrs = (C.c_void_p * 2)(None, None)
    out = (C.c_int64 * 4)()
    assert L.fheram_bank_read_list(None, members, addrs, 2, out) == ST_INVALID_ARG
    assert L.fheram_bank_read_list(None, None, addrs, 2, out) == ST_INVALID_ARG
    assert L.fheram_bank_read_list(None, members, None, 2, out) == ST_INVALID_ARG
    assert L.fheram_bank_read_list(None, None, None, 0, None) == ST_INVALID_ARG
    assert L.fheram_bank_read_list_result(None, 0, 1, out) == ST_INVALID_ARG
    assert L.fheram_bank_read_list_result(None, 0, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_read_list_result(None, -1, 0, None) == ST_INVALID_ARG


def test_the_mirrors_exist():
    pkg = load_package()
    assert callable(pkg.RamBank.read_list) and callable(pkg.RamBank.list_result)
    hpp = open(os.path.join(ROOT, "fhe-ram_amd", "host", "fheram.hpp")).read()
    bank = hpp[hpp.index("class Bank {"):]
    assert re.search(r"\bread_list\s*\(", bank) and "fheram_bank_read_list(" in bank
    assert re.search(r"\blist_result\s*\(", bank) and "fheram_bank_read_list_result(" in bank
    assert "read_list(" in open(os.path.join(ROOT, "fhe-ram_amd", "host", "host_check.cpp")).read()
    rust = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn fheram_bank_read_list(" in rust and "fn fheram_bank_read_list_result(" in rust and "FHERAM_READ_LIST_MAX" in rust
