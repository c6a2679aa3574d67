"""The register files of a bank (include/fheram.h: fheram_bank_regs_*) as far as a box without a GPU can see them: the declarations, the
exports, the bound signatures, the two new source kinds, what a null bank or register file returns, the refusals the Python mirror makes
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
NAMES = ["fheram_bank_regs_create", "fheram_regs_destroy", "fheram_regs_bits", "fheram_bank_regs_state", "fheram_bank_regs_upload",
         "fheram_bank_regs_download", "fheram_bank_regs_pack", "fheram_bank_regs_read", "fheram_bank_regs_result",
         "fheram_bank_regs_read_prepare_write", "fheram_bank_regs_old_result", "fheram_bank_regs_write"]


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
    assert "typedef struct fheram_regs fheram_regs;" in code
    # the signatures, as the header gives them
    I64P, VP, SRC = C.POINTER(C.c_int64), C.c_void_p, pkg.api._CSelectSrc
    want = {"fheram_bank_regs_create": (C.c_int, [VP, C.c_int, C.POINTER(VP)]), "fheram_regs_destroy": (None, [VP]),
            "fheram_regs_bits": (C.c_int, [VP]), "fheram_bank_regs_state": (C.c_int, [VP, VP]),
            "fheram_bank_regs_upload": (C.c_int, [VP, VP, I64P]), "fheram_bank_regs_download": (C.c_int, [VP, VP, I64P]),
            "fheram_bank_regs_pack": (C.c_int, [VP, VP, C.c_int, C.POINTER(SRC), I64P]),
            "fheram_bank_regs_read": (C.c_int, [VP, VP, C.POINTER(VP), C.c_int, I64P]),
            "fheram_bank_regs_result": (C.c_int, [VP, C.c_int, C.c_int, I64P]),
            "fheram_bank_regs_read_prepare_write": (C.c_int, [VP, VP, VP, I64P]), "fheram_bank_regs_old_result": (C.c_int, [VP, I64P]),
            "fheram_bank_regs_write": (C.c_int, [VP, VP, VP, SRC, I64P])}
    for name, (res, args) in want.items():
        assert bound[name][1] is res and list(bound[name][2]) == args, name
        assert getattr(lib, name).argtypes == args, name


def test_the_two_source_kinds(pkg):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"#define\s+FHERAM_SRC_REGS_RESULT\s+5\b", code) and re.search(r"#define\s+FHERAM_SRC_REGS_OLD\s+6\b", code)
    assert (pkg.api.SRC_REGS_RESULT, pkg.api.SRC_REGS_OLD) == (5, 6)
    S, L = pkg.Src, pkg.Lane
    assert (S.regs(3).kind, S.regs(3).index) == (5, 3) and (S.regs_old().kind, S.regs_old().index) == (6, 0)
    assert L.regs(2, 1) == L(5, 2, 1) and L.regs_old(3) == L(6, 0, 3)
    assert L.of(S.regs(1), 2) == L.regs(1, 2) and L.of(S.regs_old(), 0) == L.regs_old(0)


def test_null_bank_and_null_register_file(pkg):
    lib = pkg.library()
    out = C.c_void_p(1)
    src = pkg.api._CSelectSrc(0, 0)
    assert lib.fheram_bank_regs_create(None, 5, C.byref(out)) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_upload(None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_download(None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_pack(None, None, 1, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_read(None, None, None, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_result(None, 0, 1, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_read_prepare_write(None, None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_old_result(None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_write(None, None, None, src, None) == ST_INVALID_ARG
    assert lib.fheram_bank_regs_state(None, None) == 0
    assert lib.fheram_regs_bits(None) == 0
    lib.fheram_regs_destroy(None)


def test_the_python_mirror_refuses_before_the_library(pkg):
    params = pkg.Parameters(max_addr=1 << 12, word_size=2)
    bank = types.SimpleNamespace(params=params, _h=None, _host_words=lambda hw, slots: pkg.RamBank._host_words(bank, hw, slots))
    rf = pkg.RegFile(bank, None, 3)
    S = pkg.Src

    def refused(call, say):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG and say in e.value.msg, e.value

    refused(lambda: rf.read([]), "at least one Selector")
    refused(lambda: rf.read([object()]), "takes a Selector")
    refused(lambda: rf.read_prepare_write(None), "takes a Selector")
    refused(lambda: rf.write(None, S.zero()), "takes a Selector")
    refused(lambda: rf.pack([]), "non-empty list of Src")
    refused(lambda: rf.pack([(0, 0)]), "non-empty list of Src")
    refused(lambda: rf.load(np.zeros(7, dtype=np.int64)), "invalid data")
    refused(lambda: rf.pack([S.host(2)], host_words=np.zeros((2, 2, params.glwe_len()), dtype=np.int64)), "outside host_words")
    sel = object.__new__(pkg.Selector)
    refused(lambda: rf.write(sel, (1, 0)), "as a Src")
    refused(lambda: rf.write(sel, S.host(1), host_words=np.zeros((1, 2, params.glwe_len()), dtype=np.int64)), "outside host_words")


def test_the_cpp_mirror_compiles_and_drives_every_call():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(host, "host_check.cpp")])
    mirror, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    for name in NAMES:
        assert name + "(" in mirror, f"Bank::RegFile does not call {name}"
    for call in ("B::RegFile", ".load(", ".store()", ".pack(", ".read(", ".result(", ".read_prepare_write(", ".old_result()", ".write(", ".state()", ".bits()"):
        assert call in check, f"host_check.cpp does not drive {call}"
