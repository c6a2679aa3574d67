"""The C ABI of the derive list (include/fheram.h: fheram_bank_derive_list, fheram_bank_address_download): both symbols are declared,
exported and bound with their signatures, the item struct and the two limits are mirrored, null handles are refused, and the Python mirror
refuses malformed calls before it reaches the library.  No compute calls: this runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P = C.POINTER(C.c_int64)
VP = C.c_void_p
ST_INVALID_ARG = 1


def _signatures(pkg):
    return {
        "fheram_bank_derive_list": (C.c_int, [VP, C.POINTER(pkg.api._CDeriveItem), C.c_int]),
        "fheram_bank_address_download": (C.c_int, [VP, VP, I64P]),
    }


def _header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


def _lib(pkg):
    import __graft_entry__ as ge
    if not os.path.exists(pkg.library_path()):
        ge.build()
    return pkg.library()


def _hollow_bank(pkg):
    """a RamBank without a device: only the argument checks of the mirror are reached"""
    bank = pkg.RamBank.__new__(pkg.RamBank)
    bank.params, bank.n_members, bank._h, bank._keys = pkg.Parameters(max_addr=1 << 12, word_size=4), 1, None, None
    return bank


def test_both_symbols_are_declared_exported_and_bound_with_their_signatures():
    pkg = load_package()
    lib = _lib(pkg)
    bound = {name: (res, args) for name, res, args in pkg.api._SYMBOLS}
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, (res, args) in _signatures(pkg).items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in include/fheram.h"
        assert len(m.group(1).split(",")) == len(args), (name, m.group(1))
        assert name in bound, f"{name} is not bound in api.py"
        assert bound[name][0] is res and list(bound[name][1]) == args, (name, bound[name])
        f = getattr(lib, name)   # AttributeError: not exported
        assert f.restype is res and list(f.argtypes) == args, name
    assert re.search(r"int fheram_bank_derive_list\(fheram_bank\* bank, const fheram_derive_item\* items, int n\);", code)
    assert re.search(r"int fheram_bank_address_download\(fheram_bank\* bank, const fheram_addr\* addr, int64_t\* out\);", code)


def test_struct_and_constants_are_mirrored():
    pkg = load_package()
    h, a = _header(), pkg.api
    assert int(re.search(r"#define\s+FHERAM_DERIVE_LIST_MAX\s+(\d+)", h).group(1)) == a.DERIVE_LIST_MAX == 32
    assert int(re.search(r"#define\s+FHERAM_DERIVE_LIST_DIGITS_MAX\s+(\d+)", h).group(1)) == a.DERIVE_LIST_DIGITS_MAX == 64
    for name, value in (("ADDRESS", a.DERIVE_ADDRESS), ("SELECTOR", a.DERIVE_SELECTOR), ("FIELD", a.DERIVE_FIELD)):
        assert int(re.search(r"FHERAM_DERIVE_" + name + r"\s*=\s*(\d+)", h).group(1)) == value
    body = re.search(r"typedef struct fheram_derive_item \{(.*?)\} fheram_derive_item;", h, flags=re.S)
    assert body
    decl = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    assert re.sub(r"\s+", " ", decl).strip() == "int32_t kind, first_bit; int32_t sign; int32_t field; const fheram_fheuint* fu; void* target;"
    assert [(f, t) for f, t in a._CDeriveItem._fields_] == [("kind", C.c_int32), ("first_bit", C.c_int32), ("sign", C.c_int32), ("field", C.c_int32),
                                                              ("fu", C.c_void_p), ("target", C.c_void_p)]
    assert C.sizeof(a._CDeriveItem) == 32
    assert a._CDeriveItem.fu.offset == 16 and a._CDeriveItem.target.offset == 24
    assert pkg.Derive is a.Derive


def test_null_bank_is_refused_without_a_crash():
    pkg = load_package()
    lib = _lib(pkg)
    items = (pkg.api._CDeriveItem * 1)(pkg.api._CDeriveItem(0, 0, 0, 0, None, None))
    buf = (C.c_int64 * 4)()
    assert lib.fheram_bank_derive_list(None, items, 1) == ST_INVALID_ARG
    assert lib.fheram_bank_derive_list(None, None, 1) == ST_INVALID_ARG
    assert lib.fheram_bank_derive_list(None, None, 0) == ST_INVALID_ARG
    assert lib.fheram_bank_address_download(None, None, buf) == ST_INVALID_ARG
    assert lib.fheram_bank_address_download(None, None, None) == ST_INVALID_ARG


def test_python_mirror_refuses_malformed_calls_before_the_library():
    pkg = load_package()
    D = pkg.Derive
    bank = _hollow_bank(pkg)
    fu = pkg.FheUintPrepared(bank, None, 32)          # handles of nothing: no call below reaches the library
    plain = pkg.Selector(bank, None, 4)
    field = pkg.Selector(bank, None, 4)
    field.widths = [2, 2]
    addr = pkg.Address.alloc_from_params(bank.params)
    item = D.address(fu, addr, first_bit=2, sign=True)
    assert (item.kind, item.first_bit, item.sign, item.field, item.target) == (pkg.api.DERIVE_ADDRESS, 2, True, 0, addr)
    assert D.address(fu).target is None
    item = D.selector(fu, plain, first_bit=7)
    assert (item.kind, item.first_bit, item.sign, item.field, item.target) == (pkg.api.DERIVE_SELECTOR, 7, False, 0, plain)
    items = D.fields(field, [fu, fu], [0, 7])
    assert [(i.kind, i.first_bit, i.sign, i.field) for i in items] == [(pkg.api.DERIVE_FIELD, 0, False, 0), (pkg.api.DERIVE_FIELD, 7, False, 1)]
    assert all(i.target is field for i in items)
    for what, call in (
            ("address: no integer", lambda: D.address(object(), addr)),
            ("address: no Address", lambda: D.address(fu, plain)),
            ("selector: no integer", lambda: D.selector(None, plain)),
            ("selector: no Selector", lambda: D.selector(fu, addr)),
            ("selector: a field selector", lambda: D.selector(fu, field)),
            ("fields: a plain selector", lambda: D.fields(plain, [fu, fu], [0, 0])),
            ("fields: no Selector", lambda: D.fields(object(), [fu, fu], [0, 0])),
            ("fields: one integer for two widths", lambda: D.fields(field, [fu], [0, 0])),
            ("fields: three first bits for two widths", lambda: D.fields(field, [fu, fu], [0, 1, 2])),
            ("fields: no integer", lambda: D.fields(field, [fu, object()], [0, 0])),
            ("derive_list: nothing", lambda: bank.derive_list([])),
            ("derive_list: no Derive", lambda: bank.derive_list([object()])),
            ("derive_list: a list that holds no Derive", lambda: bank.derive_list([[fu, addr]])),
            ("derive_list: 33 items", lambda: bank.derive_list([D.selector(fu, plain)] * 33)),
            ("derive_list: 33 items through fields", lambda: bank.derive_list([items] * 16 + [D.selector(fu, plain)])),
            ("address_digits: no Address", lambda: bank.address_digits(plain))):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG, what
    fu._h = plain._h = field._h = None   # (nothing to destroy)


def test_cpp_mirror_has_the_entry_points_and_host_check_drives_them():
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    hpp, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for name in _signatures(load_package()):
        assert name + "(" in hpp, name
    assert ".derive_list(" in check and ".address_digits(" in check
