"""Wide register files (include/fheram.h fheram_bank_regs_create_wide, fheram_bank_regs_peek / _poke) as far as a box without
a GPU can see them: the three declarations, the exports, the bound signatures, the calls on a null bank and a null register file, the
refusals the Python mirror makes itself, and the C++ mirror, built with -Wall -Werror and run."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_INVALID_ARG = 1
NAMES = ["fheram_bank_regs_create_wide", "fheram_bank_regs_peek", "fheram_bank_regs_poke"]


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
    VP, I64P, U32P = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    decl = {
        "fheram_bank_regs_create_wide": r"fheram_bank\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*fheram_regs\s*\*\*\s*\w+",
        "fheram_bank_regs_peek": r"fheram_bank\s*\*\s*\w+\s*,\s*const\s+fheram_regs\s*\*\s*\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int64_t\s*\*\s*\w+",
        "fheram_bank_regs_poke": r"fheram_bank\s*\*\s*\w+\s*,\s*fheram_regs\s*\*\s*\w+\s*,\s*const\s+uint32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                                 r"\s*const\s+fheram_select_src\s*\*\s*\w+\s*,\s*const\s+int64_t\s*\*\s*\w+",
    }
    args = {
        "fheram_bank_regs_create_wide": [VP, C.c_int, C.POINTER(VP)],
        "fheram_bank_regs_peek": [VP, VP, U32P, C.c_int, I64P],
        "fheram_bank_regs_poke": [VP, VP, U32P, C.c_int, C.POINTER(pkg.api._CSelectSrc), I64P],
    }
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + decl[name] + r"\s*\)\s*;", code), f"{name} is not declared as the contract says"
        assert hasattr(lib, name), f"{name} is not exported"
        _, res, a = bound[name]
        assert res is C.c_int and list(a) == args[name], name
        assert getattr(lib, name).argtypes == args[name], name
    # the creator beside the narrow one, the public calls beside the members' twins
    at = {m: code.index(m) for m in ("fheram_bank_regs_create(", "fheram_bank_regs_create_wide(", "fheram_regs_destroy(", "fheram_bank_poke(",
                                     "fheram_bank_regs_peek(", "fheram_bank_regs_poke(", "fheram_bank_read_mix(")}
    assert at["fheram_bank_regs_create("] < at["fheram_bank_regs_create_wide("] < at["fheram_regs_destroy("]
    assert at["fheram_bank_poke("] < at["fheram_bank_regs_peek("] < at["fheram_bank_regs_poke("] < at["fheram_bank_read_mix("]


def test_every_declared_symbol_is_still_bound_and_no_source_kind_is_new(pkg):
    code = header()
    declared = sorted(set(re.findall(r"\b(fheram_[a-z0-9_]+)\s*\(", code)))
    assert all(n in declared for n in NAMES)
    assert sorted(pkg.api.exported_symbols()) == declared, set(declared) ^ set(pkg.api.exported_symbols())
    kinds = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(FHERAM_SRC_\w+)\s+(\d+)", code)}
    assert kinds == {"FHERAM_SRC_REGS_RESULT": 5, "FHERAM_SRC_REGS_OLD": 6, "FHERAM_SRC_TABLE_RESULT": 8, "FHERAM_SRC_PEEK_RESULT": 10}, kinds
    assert re.search(r"#define\s+FHERAM_SELECT_BITS_MAX\s+5\b", code) and re.search(r"#define\s+FHERAM_TABLE_BITS_MAX\s+12\b", code)
    assert re.search(r"#define\s+FHERAM_SELECTOR_WIDE_DIGITS_MAX\s+5\b", code)
    # the buffers of a register file stay tied to the wide selectors' digit limit
    regs = open(os.path.join(ROOT, "fhe-ram_amd", "csrc", "regs.hpp")).read()
    assert re.search(r"static_assert\(\s*REGS_DIGITS_MAX\s*==\s*FHERAM_SELECTOR_WIDE_DIGITS_MAX", regs)


def test_null_bank_and_null_register_file(pkg):
    lib = pkg.library()
    out = C.c_void_p(1)
    idx = (C.c_uint32 * 1)(0)
    word = np.zeros(16, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    src = (pkg.api._CSelectSrc * 1)(pkg.api._CSelectSrc(0, 0))
    assert lib.fheram_bank_regs_create_wide(None, 12, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_create_wide(None, 12, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_peek(None, None, idx, 1, word) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_peek(None, None, None, 0, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_poke(None, None, idx, 1, src, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_poke(None, None, None, 0, None, None) == ST_INVALID_ARG
    assert lib.fheram_regs_bits(None) == 0
    lib.fheram_regs_destroy(None)


def test_the_python_mirror_refuses_before_the_library(pkg):
    params = pkg.Parameters(max_addr=1 << 12, word_size=4)
    bank = types.SimpleNamespace(params=params, _h=None, n_members=2)
    bank._host_words = lambda *a: pkg.RamBank._host_words(bank, *a)
    S = pkg.Src
    word = np.zeros((1, 4, params.glwe_len()), dtype=np.int64)

    def refused(call, say):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG and say in e.value.msg, e.value

    refused(lambda: pkg.RamBank.scratch(bank, 0), "bits = 0 is outside [1, TABLE_BITS_MAX = 12]")
    refused(lambda: pkg.RamBank.scratch(bank, 13), "bits = 13 is outside [1, TABLE_BITS_MAX = 12]")
    rf = pkg.RegFile(bank, None, 12)
    refused(lambda: rf.peek([]), "1 to PEEK_MAX = 16 indices")
    refused(lambda: rf.peek([0] * 17), "1 to PEEK_MAX = 16 indices")
    refused(lambda: rf.poke(list(range(17)), srcs=[S.zero()] * 17), "1 to PEEK_MAX = 16 indices")
    refused(lambda: rf.peek([4096]), "outside the register file's 2^bits = 4096 words")
    refused(lambda: rf.peek([-1]), "outside the register file's 2^bits = 4096 words")
    refused(lambda: rf.poke([7, 4095, 7], srcs=[S.zero()] * 3), "distinct")
    refused(lambda: rf.poke([7]), "takes words, or srcs")
    refused(lambda: rf.poke([7], words=word[:, :3]), "GLWEs of words")
    refused(lambda: rf.poke([7], srcs=[S.zero(), S.zero()]), "one Src per entry")
    refused(lambda: rf.poke([7], srcs=[object()]), "one Src per entry")
    refused(lambda: rf.poke([7], srcs=[S.host(0)]), "a host source needs words")
    refused(lambda: rf.poke([7], words=word, srcs=[S.host(16)]), "host slots [0, PEEK_MAX = 16)")
    refused(lambda: rf.poke([7], words=word, srcs=[S.host(1)]), "outside host_words")
    refused(lambda: rf.load_plain(np.zeros(4095 * 4, dtype=np.uint8)), "2^bits * word_size = 16384 bytes")
    narrow = pkg.RegFile(bank, None, 5)
    refused(lambda: narrow.peek([32]), "outside the register file's 2^bits = 32 words")
    wide = types.SimpleNamespace(params=pkg.Parameters(max_addr=1 << 12, word_size=8), _h=None, n_members=2)
    refused(lambda: pkg.RegFile(wide, None, 12).peek([0] * 9), "n * word_size = 72 exceeds 64")


def test_the_cpp_mirror_builds_runs_and_drives_every_call(pkg, tmp_path):
    """on a box without a GPU host_check ends with the C ABI's DEVICE status, loudly, and exits 0; with one it runs the scratch block"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    exe, libdir = str(tmp_path / "host_check"), os.path.dirname(pkg.library_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(host, "host_check.cpp"), "-L" + libdir, "-lfheram", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    mirror, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for name in NAMES:
        assert name + "(" in mirror, f"the C++ mirror does not call {name}"
    for call in (".scratch(12)", ".peek({7, 4095}", ".poke({7, 2048}", "B::RegFile six(lists, 6)"):
        assert call in check, f"host_check.cpp does not drive {call}"
