"""The public side of a bank (include/fheram.h "THE PUBLIC SIDE of a bank") as far as a box without a GPU can see it: the five
declarations, the exports, the bound signatures, the new source kind, the calls on a null bank, the refusals the Python mirror makes
itself, and the C++ mirror, compiled with -Wall -Werror, whose check program drives the calls."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_INVALID_ARG = 1
NAMES = ["fheram_bank_ram_load_plain", "fheram_bank_regs_load_plain", "fheram_bank_peek", "fheram_bank_peek_result", "fheram_bank_poke",
         "fheram_bank_selftest_fail_public_alloc"]


def header(strip=True):
    src = open(os.path.join(ROOT, "include", "fheram.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S) if strip else src


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.library_path()):
        import __graft_entry__ as ge
        ge.build()
    return p


def test_declared_exported_and_bound(pkg):
    code = header()
    lib = pkg.library()
    bound = {s[0]: s for s in pkg.api._SYMBOLS}
    VP, I64P, U8P, U64P, IP = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    decl = {
        "fheram_bank_ram_load_plain": r"fheram_bank\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*size_t\s+\w+\s*,\s*size_t\s+\w+\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*,\s*size_t\s+\w+",
        "fheram_bank_regs_load_plain": r"fheram_bank\s*\*\s*\w+\s*,\s*fheram_regs\s*\*\s*\w+\s*,\s*const\s+uint8_t\s*\*\s*\w+\s*,\s*size_t\s+\w+",
        "fheram_bank_peek": r"fheram_bank\s*\*\s*\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int64_t\s*\*\s*\w+",
        "fheram_bank_peek_result": r"fheram_bank\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int64_t\s*\*\s*\w+",
        "fheram_bank_poke": r"fheram_bank\s*\*\s*\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                            r"\s*const\s+fheram_select_src\s*\*\s*\w+\s*,\s*const\s+int64_t\s*\*\s*\w+",
        "fheram_bank_selftest_fail_public_alloc": r"fheram_bank\s*\*\s*\w+\s*,\s*int\s+\w+",
    }
    args = {
        "fheram_bank_ram_load_plain": [VP, C.c_int, C.c_size_t, C.c_size_t, U8P, C.c_size_t],
        "fheram_bank_regs_load_plain": [VP, VP, U8P, C.c_size_t],
        "fheram_bank_peek": [VP, IP, U64P, C.c_int, I64P],
        "fheram_bank_peek_result": [VP, C.c_int, C.c_int, I64P],
        "fheram_bank_poke": [VP, IP, U64P, C.c_int, C.POINTER(pkg.api._CSelectSrc), I64P],
        "fheram_bank_selftest_fail_public_alloc": [VP, C.c_int],
    }
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + decl[name] + r"\s*\)\s*;", code), f"{name} is not declared as the contract says"
        assert hasattr(lib, name), f"{name} is not exported"
        _, res, a = bound[name]
        assert res is C.c_int and list(a) == args[name], name
        assert getattr(lib, name).argtypes == args[name], name
    # beside the tables, in front of the mixed reads
    at = {m: code.index(m) for m in ("fheram_bank_table_selector_alloc_fields(", "fheram_bank_ram_load_plain(", "fheram_bank_poke(", "fheram_bank_read_mix(")}
    assert at["fheram_bank_table_selector_alloc_fields("] < at["fheram_bank_ram_load_plain("] < at["fheram_bank_poke("] < at["fheram_bank_read_mix("]
    assert "CONTRACT-COMPATIBLE ONLY" in header(False)[header(False).index("THE PUBLIC SIDE of a bank"):header(False).index("FHERAM_PEEK_MAX")]


def test_every_declared_symbol_is_still_bound(pkg):
    declared = sorted(set(re.findall(r"\b(fheram_[a-z0-9_]+)\s*\(", header())))
    assert all(n in declared for n in NAMES)
    assert sorted(pkg.api.exported_symbols()) == declared, set(declared) ^ set(pkg.api.exported_symbols())


def test_the_new_source_kind_and_the_limit(pkg):
    """a macro beside the FHERAM_SRC_* enum as the register files' and the tables' kinds are; it takes the first number no caller relies on
    being refused (7 and 9 are pinned as unknown kinds)"""
    code = header()
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FHERAM_SRC_\w+)\s+(\d+)", code)}
    assert kinds == {"FHERAM_SRC_REGS_RESULT": 5, "FHERAM_SRC_REGS_OLD": 6, "FHERAM_SRC_TABLE_RESULT": 8, "FHERAM_SRC_PEEK_RESULT": 10}, kinds
    assert re.search(r"#define\s+FHERAM_PEEK_MAX\s+16\b", code)
    assert pkg.api.SRC_PEEK_RESULT == 10 and pkg.api.PEEK_MAX == 16
    s, l = pkg.Src.peek(3), pkg.Lane.peek(2, 1)
    assert (s.kind, s.index) == (10, 3) and (l.kind, l.index, l.lane, l.reserved) == (10, 2, 1, 0)
    assert pkg.Lane.of(s, 1) == pkg.Lane.peek(3, 1)
    mirror = open(os.path.join(ROOT, "fhe-ram_amd", "host", "fheram.hpp")).read()
    assert "src_peek(int output) { return {FHERAM_SRC_PEEK_RESULT, output}; }" in mirror


def test_null_bank(pkg):
    lib = pkg.library()
    data = (C.c_uint8 * 8)()
    mem, adr = (C.c_int * 1)(0), (C.c_uint64 * 1)(0)
    out = np.zeros(16, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    src = (pkg.api._CSelectSrc * 1)(pkg.api._CSelectSrc(0, 0))
    assert lib.fheram_bank_ram_load_plain(None, 0, 0, 1, data, 8) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_load_plain(None, None, data, 8) == ST_INVALID_ARG
    assert lib.fheram_bank_peek(None, mem, adr, 1, out) == ST_INVALID_ARG
    assert lib.fheram_bank_peek(None, None, None, 0, None) == ST_INVALID_ARG
    assert lib.fheram_bank_peek_result(None, 0, 1, out) == ST_INVALID_ARG
    assert lib.fheram_bank_poke(None, mem, adr, 1, src, None) == ST_INVALID_ARG
    assert lib.fheram_bank_selftest_fail_public_alloc(None, 1) == ST_INVALID_ARG


def test_the_python_mirror_refuses_before_the_library(pkg):
    params = pkg.Parameters(max_addr=(1 << 12) + 512, word_size=4)
    bank = types.SimpleNamespace(params=params, _h=None, n_members=2)
    bank._member = lambda m: pkg.RamBank._member(bank, m)
    bank._public_entries = lambda *a: pkg.RamBank._public_entries(bank, *a)
    bank._host_words = lambda *a: pkg.RamBank._host_words(bank, *a)
    rf = pkg.RegFile(bank, None, 5)
    load, peek, poke = pkg.RamBank.load_plain, pkg.RamBank.peek, pkg.RamBank.poke
    S = pkg.Src
    word = np.zeros((1, 4, params.glwe_len()), dtype=np.int64)

    def refused(call, say):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG and say in e.value.msg, e.value

    refused(lambda: load(bank, 2, np.zeros(4608 * 4, dtype=np.uint8)), "outside the bank's 2 members")
    refused(lambda: load(bank, 0, np.zeros(0, dtype=np.uint8)), "not a positive number of words")
    refused(lambda: load(bank, 0, np.zeros(4096 * 4 + 3, dtype=np.uint8)), "not a positive number of words")
    refused(lambda: load(bank, 0, np.zeros(100 * 4, dtype=np.uint8)), "neither fill whole rows nor end at max_addr")
    refused(lambda: load(bank, 0, np.zeros(4609 * 4, dtype=np.uint8)), "neither fill whole rows nor end at max_addr")
    refused(lambda: load(bank, 0, np.zeros(4096 * 4, dtype=np.uint8), first_row=1), "neither fill whole rows nor end at max_addr")
    refused(lambda: load(bank, 0, np.zeros(512 * 4, dtype=np.uint8), first_row=2), "outside the member's 2 rows")
    refused(lambda: rf.load_plain(np.zeros(31 * 4, dtype=np.uint8)), "2^bits * word_size = 128 bytes")
    refused(lambda: peek(bank, [], []), "1 to PEEK_MAX = 16 members")
    refused(lambda: peek(bank, [0] * 17, [0] * 17), "1 to PEEK_MAX = 16 members")
    refused(lambda: peek(bank, [0, 1], [0]), "as many addresses")
    refused(lambda: peek(bank, [2], [0]), "outside the bank's 2 members")
    refused(lambda: peek(bank, [0], [4608]), "outside max_addr = 4608")
    refused(lambda: peek(bank, [0], [-1]), "outside max_addr = 4608")
    refused(lambda: poke(bank, [0, 0], [7, 7], srcs=[S.zero(), S.zero()]), "distinct")
    refused(lambda: poke(bank, [0], [7]), "takes words, or srcs")
    refused(lambda: poke(bank, [0], [7], words=word[:, :3]), "GLWEs of words")
    refused(lambda: poke(bank, [0], [7], srcs=[S.zero(), S.zero()]), "one Src per entry")
    refused(lambda: poke(bank, [0], [7], srcs=[object()]), "one Src per entry")
    refused(lambda: poke(bank, [0], [7], srcs=[S.host(0)]), "a host source needs words")
    refused(lambda: poke(bank, [0], [7], words=word, srcs=[S.host(16)]), "host slots [0, PEEK_MAX = 16)")
    refused(lambda: poke(bank, [0], [7], words=word, srcs=[S.host(1)]), "outside host_words")
    wide = types.SimpleNamespace(params=pkg.Parameters(max_addr=1 << 12, word_size=8), _h=None, n_members=2)
    wide._member = lambda m: pkg.RamBank._member(wide, m)
    wide._public_entries = lambda *a: pkg.RamBank._public_entries(wide, *a)
    refused(lambda: peek(wide, [0] * 9, [0] * 9), "n * word_size = 72 exceeds 64")


def test_cpp_mirror_compiles_and_host_check_drives_the_calls():
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(host, "host_check.cpp")])
    mirror, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for call in ("fheram_bank_ram_load_plain(", "fheram_bank_regs_load_plain(", "fheram_bank_peek(", "fheram_bank_peek_result(", "fheram_bank_poke("):
        assert call in mirror, f"the C++ mirror does not call {call[:-1]}"
    for use in (".load_plain(1, image)", ".load_plain(lr,", ".peek(", ".peek_result(", ".poke(", "src_peek("):
        assert use in check, f"host_check.cpp does not drive {use}"
