"""fheram_bank_read_prepare_write_mix (include/fheram.h) as far as a box without a GPU can see it: the declaration, the
export, the bound signature and the struct's layout, the call on a null bank, the refusals the Python mirror makes itself, and the C++
mirror, compiled with -Wall -Werror, whose check program drives the call."""
import ctypes as C
import os
import re
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
    VP, I64P = C.c_void_p, C.POINTER(C.c_int64)
    assert re.search(r"\bint\s+fheram_bank_read_prepare_write_mix\s*\(\s*fheram_bank\s*\*\s*\w+\s*,\s*const\s+fheram_mix_reads\s*\*\s*\w+\s*,"
                     r"\s*const\s+fheram_mix_prepares\s*\*\s*\w+\s*,(\s*int64_t\s*\*\s*\w+\s*,){4}\s*int64_t\s*\*\s*\w+\s*\)\s*;", code), \
        "fheram_bank_read_prepare_write_mix is not declared with the two structs and five outputs"
    assert hasattr(lib, "fheram_bank_read_prepare_write_mix"), "fheram_bank_read_prepare_write_mix is not exported"
    name, res, args = bound["fheram_bank_read_prepare_write_mix"]
    assert res is C.c_int and list(args) == [VP, C.POINTER(pkg.api._CMixReads), C.POINTER(pkg.api._CMixPrepares)] + [I64P] * 5
    assert lib.fheram_bank_read_prepare_write_mix.argtypes == list(args)
    # the struct: field names and order as in the header; pointers and ints of the platform's sizes
    body = re.search(r"typedef\s+struct\s+fheram_mix_prepares\s*\{(.*?)\}\s*fheram_mix_prepares\s*;", code, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == ["members", "addrs", "n_list", "regs", "reg_sel"]
    assert [f[0] for f in pkg.api._CMixPrepares._fields_] == fields
    ptr, integer = C.sizeof(C.c_void_p), C.sizeof(C.c_int)
    for f in fields:
        assert getattr(pkg.api._CMixPrepares, f).size == (integer if f.startswith("n_") else ptr), f
    assert C.sizeof(pkg.api._CMixPrepares) == 5 * ptr   # four pointers and a padded int
    assert re.search(r"\bfheram_regs\s*\*\s*regs\s*;", body) and not re.search(r"const\s+fheram_regs", body), "the prepared register file is written: not const"
    # beside MIXED READS: behind fheram_bank_read_mix, in front of the bank's setup side
    at = {m: code.index(m) for m in ("fheram_bank_read_mix(", "fheram_mix_prepares {", "fheram_bank_read_prepare_write_mix(", "fheram_bank_secret_create(")}
    assert at["fheram_bank_read_mix("] < at["fheram_mix_prepares {"] < at["fheram_bank_read_prepare_write_mix("] < at["fheram_bank_secret_create("]


def test_every_declared_symbol_is_still_bound(pkg):
    declared = sorted(set(re.findall(r"\b(fheram_[a-z0-9_]+)\s*\(", header())))
    assert "fheram_bank_read_prepare_write_mix" in declared
    assert sorted(pkg.api.exported_symbols()) == declared, set(declared) ^ set(pkg.api.exported_symbols())


def test_null_bank(pkg):
    lib = pkg.library()
    reads, prepares = pkg.api._CMixReads(), pkg.api._CMixPrepares()
    assert lib.fheram_bank_read_prepare_write_mix(None, C.byref(reads), C.byref(prepares), None, None, None, None, None) == ST_INVALID_ARG
    assert lib.fheram_bank_read_prepare_write_mix(None, None, None, None, None, None, None, None) == ST_INVALID_ARG


def test_the_python_mirror_refuses_before_the_library(pkg):
    params = pkg.Parameters(max_addr=1 << 12, word_size=2)
    bank = types.SimpleNamespace(params=params, _h=None, n_members=2)
    bank._member = lambda m: pkg.RamBank._member(bank, m)
    t, rf = pkg.Table(bank, None, 12), pkg.RegFile(bank, None, 5)
    sel, addr = object.__new__(pkg.Selector), object.__new__(pkg.Address)
    mix = pkg.RamBank.read_prepare_write_mix

    def refused(call, say):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == ST_INVALID_ARG and say in e.value.msg, e.value

    refused(lambda: mix(bank), "at least one preparation")
    refused(lambda: mix(bank, tables=([t], [sel])), "at least one preparation")
    refused(lambda: mix(bank, prepare_list=([], [])), "at least one preparation")
    refused(lambda: mix(bank, prepare_list=([0, 1], [addr])), "as many addresses as prepared members")
    refused(lambda: mix(bank, tables=([t] * 7, [sel] * 7), prepare_list=([0], [addr]), prepare_regs=(rf, sel)), "at most MIX_MAX = 8")
    refused(lambda: mix(bank, tables=([t] * 8, [sel] * 8), prepare_regs=(rf, sel)), "at most MIX_MAX = 8")
    refused(lambda: mix(bank, list=([0, 1], [addr]), prepare_regs=(rf, sel)), "as many addresses as members")
    refused(lambda: mix(bank, tables=([object()], [sel]), prepare_regs=(rf, sel)), "Tables and Selectors")
    refused(lambda: mix(bank, regs=(object(), [sel]), prepare_regs=(rf, sel)), "takes a RegFile")
    refused(lambda: mix(bank, prepare_list=([0], [object()])), "must be an Address")
    refused(lambda: mix(bank, prepare_regs=(object(), sel)), "a RegFile and a Selector")
    refused(lambda: mix(bank, prepare_regs=(rf, object())), "a RegFile and a Selector")
    refused(lambda: mix(bank, prepare_list=([2], [addr])), "outside the bank's 2 members")
    refused(lambda: mix(bank, prepare_list=([1, 1], [addr, addr])), "distinct")


def test_cpp_mirror_compiles_and_host_check_names_the_call():
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(host, "host_check.cpp")])
    mirror, check = open(os.path.join(host, "fheram.hpp")).read(), open(os.path.join(host, "host_check.cpp")).read()
    assert "fheram_bank_read_prepare_write_mix(" in mirror and "PrepareMixResult read_prepare_write_mix(" in mirror, "Bank::read_prepare_write_mix does not call the C ABI"
    for say in ("takes at least one preparation", "takes at most FHERAM_MIX_MAX entries in all", "takes a register file"):
        assert say in mirror[mirror.index("PrepareMixResult read_prepare_write_mix("):], f"the C++ mirror lacks its own refusal: {say}"
    assert ".read_prepare_write_mix(" in check, "host_check.cpp does not drive Bank::read_prepare_write_mix"
