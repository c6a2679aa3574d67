"""fheram_bank_read_mix (include/fheram.h) as far as a box without a GPU can see it: the declaration, the export, the bound
signature and the struct's layout, the call on a null bank, the refusals the Python mirror makes itself, and the C++ mirror's check
program (host/host_check_mix.cpp), built and run."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_INVALID_ARG = 1


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fheram.h")).read(), flags=re.S)


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
    assert re.search(r"\bint\s+fheram_bank_read_mix\s*\(\s*fheram_bank\s*\*\s*\w+\s*,\s*const\s+fheram_mix_reads\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*\w+\s*,"
                     r"\s*int64_t\s*\*\s*\w+\s*\)\s*;", code), "fheram_bank_read_mix is not declared with a struct of the groups and three outputs"
    assert hasattr(lib, "fheram_bank_read_mix"), "fheram_bank_read_mix is not exported"
    I64P, VP = C.POINTER(C.c_int64), C.c_void_p
    name, res, args = bound["fheram_bank_read_mix"]
    assert res is C.c_int and list(args) == [VP, C.POINTER(pkg.api._CMixReads), I64P, I64P, I64P]
    assert lib.fheram_bank_read_mix.argtypes == list(args)
    assert re.search(r"#define\s+FHERAM_MIX_MAX\s+8\b", code) and pkg.api.MIX_MAX == 8
    # the struct: the three groups in the header's order, as plain pointers and counts
    body = re.search(r"typedef\s+struct\s+fheram_mix_reads\s*\{(.*?)\}\s*fheram_mix_reads\s*;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == ["members", "addrs", "n_list", "tables", "table_sels", "n_table", "regs", "reg_sels", "n_regs"], fields
    assert [f[0] for f in pkg.api._CMixReads._fields_] == fields
    ptr, integer = C.sizeof(C.c_void_p), C.sizeof(C.c_int)
    for f in fields:
        assert getattr(pkg.api._CMixReads, f).size == (integer if f.startswith("n_") else ptr), f
    assert C.sizeof(pkg.api._CMixReads) == 9 * ptr   # two pointers and a padded int per group
    # it stands behind the tables' section and in front of the bank's setup side
    at = {m: code.index(m) for m in ("fheram_bank_table_selector_alloc_fields(", "FHERAM_MIX_MAX 8", "fheram_bank_read_mix(", "fheram_bank_secret_create(")}
    assert at["fheram_bank_table_selector_alloc_fields("] < at["FHERAM_MIX_MAX 8"] < at["fheram_bank_read_mix("] < at["fheram_bank_secret_create("]


def test_every_declared_symbol_is_still_bound(pkg):
    """what test_library_abi.py asks of the whole header, with the new entry point in it"""
    declared = sorted(set(re.findall(r"\b(fheram_[a-z0-9_]+)\s*\(", header())))
    assert "fheram_bank_read_mix" in declared
    assert sorted(pkg.api.exported_symbols()) == declared, set(declared) ^ set(pkg.api.exported_symbols())


def test_null_bank_and_null_reads(pkg):
    lib = pkg.library()
    reads = pkg.api._CMixReads()
    assert lib.fheram_bank_read_mix(None, C.byref(reads), None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_read_mix(None, None, None, None, None) == ST_INVALID_ARG


def test_the_python_mirror_refuses_before_the_library(pkg):
    params = pkg.Parameters(max_addr=1 << 12, word_size=2)
    bank = types.SimpleNamespace(params=params, _h=None)
    t, rf = pkg.Table(bank, None, 12), pkg.RegFile(bank, None, 5)
    sel, addr = object.__new__(pkg.Selector), object.__new__(pkg.Address)
    mix = pkg.RamBank.read_mix

    def refused(call, say):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG and say in e.value.msg, e.value

    refused(lambda: mix(bank), "all three groups are empty")
    refused(lambda: mix(bank, list=([], []), tables=([], []), regs=(rf, [])), "all three groups are empty")
    refused(lambda: mix(bank, list=([0] * 3, [addr] * 3), tables=([t] * 3, [sel] * 3), regs=(rf, [sel] * 3)), "at most MIX_MAX = 8")
    refused(lambda: mix(bank, tables=([t] * 9, [sel] * 9)), "at most MIX_MAX = 8")
    refused(lambda: mix(bank, list=([0, 1], [addr])), "as many addresses as members")
    refused(lambda: mix(bank, tables=([t, t], [sel])), "as many selectors as tables")
    refused(lambda: mix(bank, list=([0], [object()])), "must be an Address")
    refused(lambda: mix(bank, tables=([object()], [sel])), "Tables and Selectors")
    refused(lambda: mix(bank, regs=(rf, [object()])), "Tables and Selectors")
    refused(lambda: mix(bank, regs=(object(), [sel])), "takes a RegFile")


def test_the_cpp_mirror_builds_and_runs(pkg, tmp_path):
    """on a box without a GPU host_check_mix ends with the C ABI's DEVICE status, loudly, and exits 0; with one it compares a mix with the
    three single calls"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    exe, libdir = str(tmp_path / "host_check_mix"), os.path.dirname(pkg.library_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(host, "host_check_mix.cpp"), "-L" + libdir, "-lfheram", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "no GPU" in r.stdout or "bank read_mix == read_list, table_read, RegFile::read: ok" in r.stdout, r.stdout
    mirror, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check_mix.cpp")).read()
    assert "fheram_bank_read_mix(" in mirror and "MixResult read_mix(" in mirror, "Bank::read_mix does not call fheram_bank_read_mix"
    for call in (".read_mix(", ".list_result(", ".table_result(", "rf.result(", "B::src_list(", "B::src_table(", "B::src_regs("):
        assert call in check, f"host_check_mix.cpp does not drive {call}"
