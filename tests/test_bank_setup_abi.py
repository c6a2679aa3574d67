"""The setup side of a bank (include/fheram.h "Setup side of a bank") without a GPU: every entry point is declared,
exported and bound; every call refuses a null bank; the Python mirror's own refusals; the C++ mirror builds with the new methods.
(The null secret / null object refusals need a bank, so they are in tests/test_gpu_bank_setup.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _pkg import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fheram_bank_secret_create", "fheram_bank_keys_encrypt_sk", "fheram_bank_address_encrypt_sk", "fheram_bank_fheuint_encrypt_sk",
         "fheram_bank_glwe_encrypt_sk", "fheram_bank_glwe_decrypt", "fheram_bank_ram_encrypt_sk", "fheram_bank_regs_encrypt_sk",
         "fheram_bank_table_encrypt_sk", "fheram_bank_selector_encrypt_sk", "fheram_bank_source_decrypt", "fheram_bank_ram_decrypt",
         "fheram_bank_regs_decrypt", "fheram_bank_table_decrypt"]
ST_INVALID_ARG = 1


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    if not os.path.exists(p.library_path()):
        import __graft_entry__ as ge
        ge.build()
    return p


def test_every_entry_point_is_declared_exported_and_bound(pkg):
    src = open(os.path.join(ROOT, "include", "fheram.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fheram_[a-z0-9_]+)\s*\(", src))
    bound = set(pkg.api.exported_symbols())
    lib = pkg.library()
    for name in NAMES:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert {n for n in declared if n.endswith(("_encrypt_sk", "_decrypt")) and n.startswith("fheram_bank_")} == set(NAMES) - {"fheram_bank_secret_create"}


def test_every_call_refuses_a_null_bank(pkg):
    L = pkg.library()
    out = C.c_void_p(7)
    z = np.zeros(8, dtype=np.int64)
    zp = z.ctypes.data_as(C.POINTER(C.c_int64))
    b8 = np.zeros(8, dtype=np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    i32 = np.zeros(8, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    src = (pkg.api._CSelectSrc * 1)(pkg.api._CSelectSrc(2, 0))
    d = C.c_double()
    calls = [lambda: L.fheram_bank_secret_create(None, zp, C.byref(out)),
             lambda: L.fheram_bank_keys_encrypt_sk(None, None, zp, zp, None),
             lambda: L.fheram_bank_address_encrypt_sk(None, None, 0, zp, zp, C.byref(out)),
             lambda: L.fheram_bank_fheuint_encrypt_sk(None, None, 0, 8, zp, zp, C.byref(out)),
             lambda: L.fheram_bank_glwe_encrypt_sk(None, None, 1, 3, 51, None, 0, 0, zp, zp, zp),
             lambda: L.fheram_bank_glwe_decrypt(None, None, 1, 3, zp, zp),
             lambda: L.fheram_bank_ram_encrypt_sk(None, 0, None, b8, 8, zp, zp),
             lambda: L.fheram_bank_regs_encrypt_sk(None, None, None, b8, 8, zp, zp),
             lambda: L.fheram_bank_table_encrypt_sk(None, None, None, b8, 8, zp, zp),
             lambda: L.fheram_bank_selector_encrypt_sk(None, None, None, 0, zp, zp),
             lambda: L.fheram_bank_source_decrypt(None, None, src, 1, None, zp, None),
             lambda: L.fheram_bank_ram_decrypt(None, 0, None, i32, C.byref(d)),
             lambda: L.fheram_bank_regs_decrypt(None, None, None, i32, C.byref(d)),
             lambda: L.fheram_bank_table_decrypt(None, None, None, i32, C.byref(d))]
    assert len(calls) == len(NAMES)
    for name, call in zip(NAMES, calls):
        assert call() == ST_INVALID_ARG, name
    L.fheram_secret_destroy(None)   # (as every destroy: a null handle is nothing to free)


def test_python_mirror_refusals(pkg):
    """the mirror's own checks come before any library call: a bank that was never created on a device is enough to reach them"""
    bank = object.__new__(pkg.RamBank)
    bank.params, bank.n_members, bank._h, bank._keys = pkg.Parameters(max_addr=1 << 13, word_size=2), 2, None, None
    not_a_secret = np.zeros(4096, dtype=np.int64)

    class Src0:
        def uniform_limbs(self, count):
            return np.zeros(count, dtype=np.int64)

        def gaussian(self, count, scale):
            return np.zeros(count, dtype=np.int64)
    data = np.zeros((1 << 13) * 2, dtype=np.uint8)
    for call in (lambda: bank.encrypt_sk(0, data, not_a_secret, Src0(), Src0()),
                 lambda: bank.decrypt(0, not_a_secret),
                 lambda: bank.decrypt_sources(not_a_secret, [pkg.Src.member(0)]),
                 lambda: bank.glwe_decrypt(not_a_secret, np.zeros(6 * 4096, dtype=np.int64)),
                 lambda: pkg.RegFile(bank, None, 5).encrypt_sk(np.zeros(64, dtype=np.uint8), not_a_secret, Src0(), Src0()),
                 lambda: pkg.RegFile(bank, None, 5).decrypt(not_a_secret),
                 lambda: pkg.Table(bank, None, 7).encrypt_sk(np.zeros(256, dtype=np.uint8), not_a_secret, Src0(), Src0()),
                 lambda: pkg.Table(bank, None, 7).decrypt(not_a_secret),
                 lambda: pkg.Selector(bank, None, 3).encrypt_sk(1, not_a_secret, Src0(), Src0())):
        with pytest.raises(pkg.FheRamError, match="GLWESecret") as e:
            call()
        assert e.value.code == ST_INVALID_ARG
    sk = object.__new__(pkg.GLWESecret)
    sk.ram, sk._h = bank, None
    with pytest.raises(pkg.FheRamError, match="non-empty list of Src"):
        bank.decrypt_sources(sk, [])
    with pytest.raises(pkg.FheRamError, match="non-empty list of Src"):
        bank.decrypt_sources(sk, [0])
    with pytest.raises(pkg.FheRamError, match="wants must hold 2 x 2"):
        bank.decrypt_sources(sk, [pkg.Src.member(0), pkg.Src.member(1)], wants=[1, 2, 3])
    with pytest.raises(pkg.FheRamError, match="outside the bank's 2 members"):
        bank.decrypt(2, sk)
    with pytest.raises(pkg.FheRamError, match="outside the bank's 2 members"):
        bank.encrypt_sk(-1, data, sk, Src0(), Src0())
    for value in (-1, 1 << 32):
        with pytest.raises(pkg.FheRamError, match="unsigned 32-bit"):
            pkg.Selector(bank, None, 3).encrypt_sk(value, sk, Src0(), Src0())


def test_cpp_mirror_has_the_setup_side_and_builds(pkg, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    host = os.path.join(ROOT, "fhe-ram_amd", "host")
    hpp = open(os.path.join(host, "fheram.hpp")).read()
    check = open(os.path.join(host, "host_check.cpp")).read()
    for name in NAMES:
        assert name + "(" in hpp, name
    for method in ("B::Secret bsk", "sb.encrypt_keys(", "sb.encrypt_sk(", "rf.encrypt_sk(", "tb.encrypt_sk(", "sb.encrypt_address(", "B::FheUintPrepared bfu(sb, 778u",
                   "s5.encrypt_sk(", "sb.decrypt_sources(", "sb.decrypt(1, bsk", "rf.decrypt(", "tb.decrypt(", "sb.encrypt_word("):
        assert method in check, method
    exe = str(tmp_path / "host_check")
    libdir = os.path.dirname(pkg.library_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(host, "host_check.cpp"), "-L" + libdir, "-lfheram", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    if "no GPU" not in r.stdout:
        assert "bank setup side:" in r.stdout and "decrypt on the device: ok" in r.stdout, r.stdout
