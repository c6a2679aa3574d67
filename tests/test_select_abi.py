"""The C ABI of the oblivious select (include/fheram.h: fheram_bank_selector_*, fheram_bank_select, fheram_bank_select_result,
fheram_bank_write_list_selected): every symbol is declared, exported and bound with its signature, the constants are mirrored, and
null handles are refused.  No compute calls: this runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P = C.POINTER(C.c_int64)
VP, VPP, IP = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)
ST_INVALID_ARG = 1


def _signatures(pkg):
    src = pkg.api._CSelectSrc
    return {
        "fheram_bank_selector_alloc": (C.c_int, [VP, C.c_int, VPP]),
        "fheram_bank_selector_create": (C.c_int, [VP, C.POINTER(I64P), C.c_int, C.c_int, VPP]),
        "fheram_bank_selector_derive": (C.c_int, [VP, VPP, IP, C.c_int, VPP]),
        "fheram_bank_selector_download": (C.c_int, [VP, VP, I64P]),
        "fheram_selector_n_digits": (C.c_int, [VP]),
        "fheram_selector_destroy": (None, [VP]),
        "fheram_bank_select": (C.c_int, [VP, VPP, IP, C.c_int, C.POINTER(src), I64P, I64P]),
        "fheram_bank_select_result": (C.c_int, [VP, C.c_int, C.c_int, I64P]),
        "fheram_bank_write_list_selected": (C.c_int, [VP, IP, VPP, C.c_int, IP]),
    }


def _header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


def _lib(pkg):
    import __graft_entry__ as ge
    if not os.path.exists(pkg.library_path()):
        ge.build()
    return pkg.library()


def test_every_select_symbol_is_declared_exported_and_bound_with_its_signature():
    pkg = load_package()
    lib = _lib(pkg)
    bound = {name: (res, args) for name, res, args in pkg.api._SYMBOLS}
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, (res, args) in _signatures(pkg).items():
        m = re.search(r"\b(int|void)\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in include/fheram.h"
        assert (m.group(1) == "void") == (res is None), name
        assert len(m.group(2).split(",")) == len(args), (name, m.group(2))
        assert name in bound, f"{name} is not bound in api.py"
        assert bound[name][0] is res and list(bound[name][1]) == args, (name, bound[name])
        f = getattr(lib, name)   # AttributeError: not exported
        assert f.restype is res and list(f.argtypes) == args, name


def test_constants_and_source_kinds_are_mirrored():
    pkg = load_package()
    h = _header()
    assert int(re.search(r"#define\s+FHERAM_SELECT_BITS_MAX\s+(\d+)", h).group(1)) == pkg.api.SELECT_BITS_MAX == 5
    assert int(re.search(r"#define\s+FHERAM_SELECT_MAX\s+(\d+)", h).group(1)) == pkg.api.SELECT_MAX == 8
    kinds = {k: int(v) for k, v in re.findall(r"FHERAM_SRC_([A-Z_]+)\s*=\s*(\d+)", h)}
    assert kinds == {"ZERO": 0, "HOST": 1, "MEMBER_RESULT": 2, "LIST_RESULT": 3, "SELECT_RESULT": 4}
    a = pkg.api
    assert (a.SRC_ZERO, a.SRC_HOST, a.SRC_MEMBER_RESULT, a.SRC_LIST_RESULT, a.SRC_SELECT_RESULT) == (0, 1, 2, 3, 4)
    assert [(f, t) for f, t in a._CSelectSrc._fields_] == [("kind", C.c_int32), ("index", C.c_int32)] and C.sizeof(a._CSelectSrc) == 8
    S = pkg.Src
    assert [(s.kind, s.index) for s in (S.zero(), S.host(3), S.member(2), S.list(5), S.select(1))] == [(0, 0), (1, 3), (2, 2), (3, 5), (4, 1)]


def test_null_bank_selector_and_out_are_refused():
    pkg = load_package()
    lib = _lib(pkg)
    out = C.c_void_p()
    buf = (C.c_int64 * 4)()
    one, ptr = (C.c_int * 1)(1), (C.c_void_p * 1)(None)
    src = (pkg.api._CSelectSrc * 1)(pkg.api._CSelectSrc(0, 0))
    dig = (I64P * 1)(C.cast(buf, I64P))
    assert lib.fheram_bank_selector_alloc(None, 1, C.byref(out)) == ST_INVALID_ARG and out.value is None
    assert lib.fheram_bank_selector_alloc(None, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_create(None, dig, 1, 1, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_derive(None, ptr, one, 1, ptr) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_download(None, None, buf) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_download(None, None, None) == ST_INVALID_ARG
    assert lib.fheram_selector_n_digits(None) == 0
    lib.fheram_selector_destroy(None)   # a null selector is ignored, as free(NULL)
    assert lib.fheram_bank_select(None, ptr, one, 1, src, None, buf) == ST_INVALID_ARG
    assert lib.fheram_bank_select(None, None, None, 1, None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_select_result(None, 0, 1, buf) == ST_INVALID_ARG
    assert lib.fheram_bank_select_result(None, 0, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_write_list_selected(None, one, ptr, 1, one) == ST_INVALID_ARG
    assert lib.fheram_bank_write_list_selected(None, None, None, 1, None) == ST_INVALID_ARG


def test_python_mirror_refuses_malformed_calls_before_the_library():
    """the checks RamBank.select / derive_selectors / write_list_selected make on their own arguments need no bank handle"""
    pkg = load_package()
    bank = pkg.RamBank.__new__(pkg.RamBank)   # no device: only the argument checks are reached
    bank.params, bank.n_members, bank._h, bank._keys = pkg.Parameters(max_addr=1 << 12, word_size=1), 1, None, None
    for call in (lambda: bank.select([], []), lambda: bank.select([object()], [[pkg.Src.zero()]]),
                 lambda: bank.derive_selectors([], [], []), lambda: bank.derive_selectors([object()], [0], [object()])):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG


def test_cpp_mirror_has_the_select_and_host_check_drives_it():
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    hpp, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for name in ("fheram_bank_selector_alloc", "fheram_bank_selector_create", "fheram_bank_selector_derive", "fheram_bank_select(",
                 "fheram_bank_select_result", "fheram_bank_write_list_selected"):
        assert name in hpp, name
    assert ".select(" in check and "write_selected(" in check
