"""The tables of a bank (include/fheram.h: fheram_bank_table_*) as far as a box without a GPU can see them: the declarations, the exports,
the bound signatures, the two macros and the new source kind, what a null bank or table returns, the refusals the Python mirror makes
itself, and the C++ mirror."""
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
NAMES = ["fheram_bank_table_create", "fheram_table_destroy", "fheram_table_bits", "fheram_bank_table_upload", "fheram_bank_table_download",
         "fheram_bank_table_load_plain", "fheram_bank_table_read", "fheram_bank_table_result", "fheram_bank_table_selector_alloc",
         "fheram_bank_table_selector_create", "fheram_bank_table_selector_alloc_fields"]


def header():
    return open(os.path.join(ROOT, "include", "fheram.h")).read()


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.library_path()):
        import __graft_entry__ as ge
        ge.build()
    return p


def test_declared_exported_and_bound(pkg):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.library()
    bound = {s[0]: s for s in pkg.api._SYMBOLS}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound"
    assert "typedef struct fheram_table fheram_table;" in code
    # the signatures, as the header gives them
    I64P, VP, INTP = C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int)
    want = {"fheram_bank_table_create": (C.c_int, [VP, C.c_int, C.POINTER(VP)]), "fheram_table_destroy": (None, [VP]),
            "fheram_table_bits": (C.c_int, [VP]),
            "fheram_bank_table_upload": (C.c_int, [VP, VP, I64P]), "fheram_bank_table_download": (C.c_int, [VP, VP, I64P]),
            "fheram_bank_table_load_plain": (C.c_int, [VP, VP, C.POINTER(C.c_uint8), C.c_size_t]),
            "fheram_bank_table_read": (C.c_int, [VP, C.POINTER(VP), C.POINTER(VP), C.c_int, I64P]),
            "fheram_bank_table_result": (C.c_int, [VP, C.c_int, C.c_int, I64P]),
            "fheram_bank_table_selector_alloc": (C.c_int, [VP, C.c_int, C.POINTER(VP)]),
            "fheram_bank_table_selector_create": (C.c_int, [VP, C.POINTER(I64P), C.c_int, C.c_int, C.POINTER(VP)]),
            "fheram_bank_table_selector_alloc_fields": (C.c_int, [VP, INTP, C.c_int, C.POINTER(VP)])}
    for name, (res, args) in want.items():
        assert bound[name][1] is res and list(bound[name][2]) == args, name
        assert getattr(lib, name).argtypes == args, name


def test_the_macros_and_the_source_kind(pkg):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"#define\s+FHERAM_TABLE_BITS_MAX\s+12\b", code) and re.search(r"#define\s+FHERAM_SELECTOR_WIDE_DIGITS_MAX\s+5\b", code)
    assert re.search(r"#define\s+FHERAM_SRC_TABLE_RESULT\s+8\b", code)
    assert re.search(r"#define\s+FHERAM_SELECT_BITS_MAX\s+5\b", code), "the select's bound stays"
    # the wide-digits macro sits in the selector section, the table's own in a section behind the register file's
    at = {m: code.index(m) for m in ("FHERAM_SELECT_BITS_MAX 5", "FHERAM_SELECTOR_WIDE_DIGITS_MAX 5", "fheram_bank_selector_alloc(", "fheram_bank_regs_write(", "FHERAM_TABLE_BITS_MAX 12")}
    assert at["FHERAM_SELECT_BITS_MAX 5"] < at["FHERAM_SELECTOR_WIDE_DIGITS_MAX 5"] < at["fheram_bank_selector_alloc("]
    assert at["fheram_bank_regs_write("] < at["FHERAM_TABLE_BITS_MAX 12"]
    # a macro beside the enum, whose members stay the five they were
    enum = re.search(r"enum\s*\{\s*FHERAM_SRC_ZERO[^}]*\}", code).group(0)
    assert re.findall(r"FHERAM_SRC_[A-Z_]+", enum) == ["FHERAM_SRC_ZERO", "FHERAM_SRC_HOST", "FHERAM_SRC_MEMBER_RESULT", "FHERAM_SRC_LIST_RESULT", "FHERAM_SRC_SELECT_RESULT"]
    assert (pkg.api.SRC_TABLE_RESULT, pkg.api.TABLE_BITS_MAX, pkg.api.SELECTOR_WIDE_DIGITS_MAX, pkg.api.SELECT_BITS_MAX) == (8, 12, 5, 5)
    S, L = pkg.Src, pkg.Lane
    assert (S.table(3).kind, S.table(3).index) == (8, 3)
    assert L.table(2, 1) == L(8, 2, 1) and L.of(S.table(1), 2) == L.table(1, 2)


def test_null_bank_and_null_table(pkg):
    lib = pkg.library()
    out = C.c_void_p(1)
    byte = (C.c_uint8 * 4)()
    assert lib.fheram_bank_table_create(None, 12, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_bank_table_upload(None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_table_download(None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_table_load_plain(None, None, byte, 4) == ST_INVALID_ARG
    assert lib.fheram_bank_table_read(None, None, None, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_table_result(None, 0, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_table_selector_alloc(None, 12, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_bank_table_selector_create(None, None, 4, 12, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_bank_table_selector_alloc_fields(None, None, 2, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_table_bits(None) == 0
    lib.fheram_table_destroy(None)


def test_the_python_mirror_refuses_before_the_library(pkg):
    params = pkg.Parameters(max_addr=1 << 12, word_size=2)
    bank = types.SimpleNamespace(params=params, _h=None)
    t = pkg.Table(bank, None, 9)
    assert t.bits == 9

    def refused(call, say):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG and say in e.value.msg, e.value

    refused(lambda: t.load(np.zeros(7, dtype=np.int64)), "invalid data")
    refused(lambda: t.load_plain(np.zeros(1023, dtype=np.uint8)), "2^bits * word_size = 1024 bytes")
    refused(lambda: t.load_plain(np.zeros(2048, dtype=np.uint8)), "2^bits * word_size = 1024 bytes")
    sel = object.__new__(pkg.Selector)
    read = pkg.RamBank.table_read
    refused(lambda: read(bank, [], []), "at least one Selector")
    refused(lambda: read(bank, [t, t], [sel]), "one Table per selector")
    refused(lambda: read(bank, [object()], [sel]), "Tables and Selectors")
    refused(lambda: read(bank, [t], [object()]), "Tables and Selectors")


def test_the_cpp_mirror_builds_runs_and_drives_every_call(pkg, tmp_path):
    """on a box without a GPU host_check ends with the C ABI's DEVICE status, loudly, and exits 0; with one it runs the table block"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    exe, libdir = str(tmp_path / "host_check"), os.path.dirname(pkg.library_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(host, "host_check.cpp"), "-L" + libdir, "-lfheram", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    mirror, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for name in NAMES:
        assert name + "(" in mirror, f"Bank::Table / Bank::Selector does not call {name}"
    for call in ("B::Table", ".load(", ".load_plain(", ".download()", ".bits()", ".table_read(", ".table_result(", "B::src_table(", "B::Selector::Wide{}"):
        assert call in check, f"host_check.cpp does not drive {call}"
