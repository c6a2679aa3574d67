"""The C ABI of the sub-word loads and stores (include/fheram.h: fheram_bank_select_lanes, fheram_bank_selector_*_fields,
fheram_address_derive_at / fheram_bank_address_derive_at): every symbol is declared, exported and bound with its signature, the struct
and the constant are mirrored, null handles are refused; and the two pure table builders, store_merge_lanes against the reference test's
c_want formula (store.rs:298-313) and load_extract_lanes against its docstring's table, on plain byte arrays where a "lane" picks a byte.
No compute calls: this runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64P = C.POINTER(C.c_int64)
VP, VPP, IP = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int)
ST_INVALID_ARG = 1
M32 = 0xFFFFFFFF


def _signatures(pkg):
    lane = pkg.api._CSelectLane
    return {
        "fheram_bank_select_lanes": (C.c_int, [VP, VPP, IP, C.c_int, C.POINTER(lane), I64P, I64P]),
        "fheram_bank_selector_alloc_fields": (C.c_int, [VP, IP, C.c_int, VPP]),
        "fheram_bank_selector_create_fields": (C.c_int, [VP, C.POINTER(I64P), C.c_int, IP, C.c_int, VPP]),
        "fheram_bank_selector_derive_fields": (C.c_int, [VP, VP, VPP, IP]),
        "fheram_address_derive_at": (C.c_int, [VP, VPP, IP, C.c_int, C.c_int, VPP]),
        "fheram_bank_address_derive_at": (C.c_int, [VP, VPP, IP, C.c_int, C.c_int, VPP]),
    }


def _header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


def _lib(pkg):
    import __graft_entry__ as ge
    if not os.path.exists(pkg.library_path()):
        ge.build()
    return pkg.library()


def test_every_symbol_is_declared_exported_and_bound_with_its_signature():
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


def test_struct_and_constant_are_mirrored():
    pkg = load_package()
    h, a = _header(), pkg.api
    assert int(re.search(r"#define\s+FHERAM_SELECT_FIELDS_MAX\s+(\d+)", h).group(1)) == a.SELECT_FIELDS_MAX == 5
    m = re.search(r"typedef struct fheram_select_lane \{ int32_t ([a-z, ]+?)(?:\s*/\*.*?\*/)?; \} fheram_select_lane;", h)
    assert m and [f.strip() for f in m.group(1).split(",")] == ["kind", "index", "lane", "reserved"]
    assert [(f, t) for f, t in a._CSelectLane._fields_] == [(f, C.c_int32) for f in ("kind", "index", "lane", "reserved")]
    assert C.sizeof(a._CSelectLane) == 16 and C.sizeof(a._CSelectSrc) == 8
    L = pkg.Lane
    got = [(l.kind, l.index, l.lane, l.reserved) for l in (L.zero(), L.host(3, 1), L.member(2, 0), L.list_entry(5, 3), L.select(1, 2))]
    assert got == [(0, 0, 0, 0), (1, 3, 1, 0), (2, 2, 0, 0), (3, 5, 3, 0), (4, 1, 2, 0)]
    assert L.of(pkg.Src.list(4), 2) == L.list_entry(4, 2) and L.of(pkg.Src.zero(), 2) == L.zero()


def test_null_handles_are_refused():
    pkg = load_package()
    lib = _lib(pkg)
    out = C.c_void_p()
    buf = (C.c_int64 * 4)()
    one, ptr = (C.c_int * 1)(1), (C.c_void_p * 1)(None)
    lane = (pkg.api._CSelectLane * 1)(pkg.api._CSelectLane(0, 0, 0, 0))
    dig = (I64P * 1)(C.cast(buf, I64P))
    assert lib.fheram_bank_select_lanes(None, ptr, one, 1, lane, None, buf) == ST_INVALID_ARG
    assert lib.fheram_bank_select_lanes(None, None, None, 1, None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_alloc_fields(None, one, 1, C.byref(out)) == ST_INVALID_ARG and out.value is None
    assert lib.fheram_bank_selector_alloc_fields(None, None, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_create_fields(None, dig, 1, one, 1, C.byref(out)) == ST_INVALID_ARG and out.value is None
    assert lib.fheram_bank_selector_derive_fields(None, None, ptr, one) == ST_INVALID_ARG
    assert lib.fheram_bank_selector_derive_fields(None, None, None, None) == ST_INVALID_ARG
    assert lib.fheram_address_derive_at(None, ptr, one, 1, 0, ptr) == ST_INVALID_ARG
    assert lib.fheram_address_derive_at(None, None, None, 1, 0, None) == ST_INVALID_ARG
    assert lib.fheram_bank_address_derive_at(None, ptr, one, 1, 0, ptr) == ST_INVALID_ARG
    assert lib.fheram_bank_address_derive_at(None, None, None, 1, 0, None) == ST_INVALID_ARG


def test_python_mirror_refuses_malformed_calls_before_the_library():
    pkg = load_package()
    bank = pkg.RamBank.__new__(pkg.RamBank)   # no device: only the argument checks are reached
    bank.params, bank.n_members, bank._h, bank._keys = pkg.Parameters(max_addr=1 << 12, word_size=4), 1, None, None
    L = pkg.Lane
    for call in (lambda: bank.select_lanes([], []), lambda: bank.select_lanes([object()], [[[L.zero()] * 4]]),
                 lambda: bank.derive_selector_fields(object(), [], []),
                 lambda: pkg.store_merge_lanes(pkg.Src.host(0), pkg.Src.host(1), word_size=2),
                 lambda: pkg.load_extract_lanes(pkg.Src.host(0), word_size=8)):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG


# ---- the table builders on plain bytes: a word is 4 bytes, least significant first; a Lane picks one of them ---------------------------------
A, B = 0xFFFFFFFF, 0xAABBCCDD   # rs2 (x) and the loaded word (y) of the reference's test (store.rs)


def _bytes(v):
    return [(v >> (8 * i)) & 0xFF for i in range(4)]


def _apply(cand, words):
    """the 32-bit value a candidate (4 lanes) assembles from `words` = {(kind, index): value}"""
    v = 0
    for w, l in enumerate(cand):
        byte = 0 if l.kind == 0 else _bytes(words[(l.kind, l.index)])[l.lane]
        v |= byte << (8 * w)
    return v


def _rotr(v, r):
    r %= 32
    return ((v >> r) | (v << (32 - r))) & M32


def _rotl(v, r):
    return _rotr(v, 32 - r % 32)


def c_want(a, b, offset, op):
    """store.rs:298-313, restated"""
    if op == 0:
        return b
    if op == 1:
        return _rotl((_rotr(b, offset << 3) & 0xFFFFFF00) | (a & 0x000000FF), offset << 3)
    if op == 2:
        return _rotl((_rotr(b, offset << 3) & 0xFFFF0000) | (a & 0x0000FFFF), offset << 3) if offset in (0, 2) else 0
    if op == 3:
        return a if offset == 0 else 0
    return 0


def test_store_merge_lanes_is_the_reference_tests_c_want():
    pkg = load_package()
    x, y = pkg.Src.list(1), pkg.Src.member(2)
    cands = pkg.store_merge_lanes(x, y)
    assert len(cands) == 14 and all(len(c) == 4 for c in cands)
    words = {(x.kind, x.index): A, (y.kind, y.index): B}
    for offset in range(4):
        for op in range(4):
            i = op + 4 * offset
            got = _apply(cands[i], words) if i < 14 else 0   # the two trailing candidates are left out: an index >= 14 selects zero
            assert got == c_want(A, B, offset, op), (offset, op, hex(got), hex(c_want(A, B, offset, op)))
    assert c_want(A, B, 3, 2) == c_want(A, B, 3, 3) == 0
    a2, b2 = 0x01020304, 0x50607080   # a second pair, with distinct bytes in x
    words = {(x.kind, x.index): a2, (y.kind, y.index): b2}
    assert [_apply(cands[op + 4 * off], words) for off in range(4) for op in range(4) if op + 4 * off < 14] == \
        [c_want(a2, b2, off, op) for off in range(4) for op in range(4) if op + 4 * off < 14]
    assert _apply(cands[1 + 4 * 1], words) == 0x50600480   # "SB at offset 1" is [y0, x0, y2, y3]


def test_load_extract_lanes_is_its_docstrings_table():
    pkg = load_package()
    y = pkg.Src.member(0)
    cands = pkg.load_extract_lanes(y)
    assert len(cands) == 14 and all(len(c) == 4 for c in cands)
    words = {(y.kind, y.index): B}
    by = _bytes(B)
    for offset in range(4):
        for op in range(4):
            i = op + 4 * offset
            got = _apply(cands[i], words) if i < 14 else 0
            if op == 0:
                want = B if offset == 0 else 0                                                   # LW
            elif op == 1:
                want = by[offset]                                                                # LBU: zero-extended
            elif op == 2:
                want = (by[offset] | by[offset + 1] << 8) if offset in (0, 2) else 0           # LHU: zero-extended
            else:
                want = 0
            assert got == want, (offset, op, hex(got), hex(want))
    assert "NO reference counterpart" in pkg.load_extract_lanes.__doc__


def test_cpp_mirror_has_the_entry_points_and_host_check_drives_them():
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    hpp, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for name in _signatures(load_package()):
        assert name + "(" in hpp, name
    assert ".select_lanes(" in check and ".derive_selector_fields(" in check and "{2})" in check
