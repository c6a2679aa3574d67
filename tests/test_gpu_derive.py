"""fheram_address_derive / Ram.derive_addresses / RamBank.derive_addresses: K addresses from K encrypted integers as ONE launch
(k_cmux_chain), into existing addresses, with no allocation and no host wait (include/fheram.h).

The contract: the digits are those of the oracle's address_from_fheuint and of the unchanged fheram_address_set_from_fheuint, bit for
bit; an address overwritten in place behaves like a newly created one in everything that follows.  Every comparison is
np.array_equal: no tolerance anywhere.  Word size 1 or 2, so that each case runs for a few seconds."""
import ctypes as C

import numpy as np
import pytest

from _pkg import load_package

pytestmark = pytest.mark.gpu

ST_OK, ST_INVALID_ARG = 0, 1
DECOMP = [3, 3, 3, 3]
PLANS = {1 << 12: [[3, 3, 3, 3]], 1 << 13: [[3, 3, 3, 3], [1]], 1 << 14: [[3, 3, 3, 3], [2]], 1 << 16: [[3, 3, 3, 3], [3, 1]]}


def lib():
    return load_package().library()


class World:
    """One secret, (optionally) one key set and one encrypted RAM at max_addr; encrypted integers and the digits the oracle derives from
    them, computed once and shared."""

    def __init__(self, po, max_addr, word_size=1, seed=0, with_ram=False):
        pkg = load_package()
        self.pkg, self.po, self.max_addr, self.ws = pkg, po, max_addr, word_size
        self.n_bits = max_addr.bit_length() - 1
        self.o = po.Oracle(po.OParams(max_addr=max_addr, word_size=word_size))
        self.sk = self.o.secret_gen(5100 + seed)
        self.params = pkg.Parameters(max_addr=max_addr, word_size=word_size)
        self._bits, self._digits, self._reads = {}, {}, {}
        self.seed = seed
        if with_ram:
            self.evk = self.o.evk_gen(self.sk, 5101 + seed, 5102 + seed)
            self.keys = pkg.EvaluationKeysPrepared.from_dict(self.evk)
            rng = np.random.default_rng(5103 + seed)
            self.data = [rng.integers(0, 256, size=max_addr * word_size, dtype=np.uint8) for _ in range(2)]
            self.rows = [self.o.ram_encrypt(d, self.sk, 5104 + seed + 10 * m, 5105 + seed + 10 * m) for m, d in enumerate(self.data)]
            self._okeys = None

    @property
    def okeys(self):
        if self._okeys is None:
            self._okeys = self.o.keys_prepare(self.evk)
        return self._okeys

    def bits(self, k):
        """the oracle's fheuint_encrypt of k: [n_bits][fheuint_ggsw_len]"""
        if k not in self._bits:
            self._bits[k] = self.o.fheuint_encrypt(k, self.n_bits, self.sk, 5200 + self.seed + 2 * (k % 997), 5201 + self.seed + 2 * (k % 997))
        return self._bits[k]

    def digits(self, k, sign=False):
        """the oracle's address_from_fheuint: [n_digits][ggsw_len]"""
        if (k, sign) not in self._digits:
            self._digits[(k, sign)] = self.o.address_from_fheuint(self.bits(k), sign=sign)
        return self._digits[(k, sign)]

    def oracle_read(self, k, m=0):
        """the oracle's Ram::read of member m's rows at the address derived from k"""
        if (k, m) not in self._reads:
            oram = self.o.ram_new()
            oram.load(self.rows[m])
            self._reads[(k, m)] = np.array(oram.read(self.o.address_new(self.digits(k)), self.okeys))
        return self._reads[(k, m)]

    def new_ram(self, m=0, config=None, load=True):
        ram = self.pkg.Ram(self.params, 0, config=config)
        if load:
            ram.load_encrypted(self.rows[m])
        return ram

    def fu(self, owner, k):
        return self.pkg.FheUintPrepared.from_host(owner, self.bits(k))


def got_digits(addr):
    addr._digits = None   # (always from the device)
    return np.stack(addr.digits)


@pytest.fixture(scope="module")
def w14(po):
    return World(po, 1 << 14, 1, seed=0, with_ram=True)


# ---- 1. plans -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_addr", sorted(PLANS))
def test_plans_both_signs_one_launch(po, max_addr):
    w = World(po, max_addr, 1, seed=max_addr.bit_length())
    pkg = w.pkg
    assert [list(b.d) for b in w.params.base2d().v] == PLANS[max_addr]
    ram = pkg.Ram(w.params, 0)
    n_digits = sum(len(c) for c in PLANS[max_addr])
    assert lib().fheram_n_digits(ram._h) == n_digits
    k = (0b1011_0110_0111_0101 | 1 << (w.n_bits - 1)) & (max_addr - 1)   # top bit set: every digit, the one-bit digits included, rotates
    fu = w.fu(ram, k)
    for sign in (False, True):
        old = got_digits(pkg.Address.set_from_fheuint(ram, fu, sign=sign))           # the unchanged entry point
        ram.profile_enable(True)
        ram.profile_reset()
        addr, = ram.derive_addresses([fu], sign=sign)
        prof = ram.profile_get("derive")
        ram.profile_enable(False)
        got = got_digits(addr)
        want = w.digits(k, sign)
        assert np.array_equal(got, want), f"{max_addr} sign={sign}: {np.count_nonzero(got != want)} limbs differ from the oracle"
        assert np.array_equal(got, old), f"{max_addr} sign={sign}: differs from fheram_address_set_from_fheuint"
        assert prof["launches"] == 1 and prof["blocks"] == n_digits * 6, prof
    m = ram.roundoff_max()
    print(f"max_addr=2^{w.n_bits}: round-off maximum after the derivations {m}")
    assert m < 0.375


# ---- 2. batch ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def singles14(w14):
    """the single derivation of each integer the batch tests use (K = 1 launches on a context of their own)"""
    ram = w14.pkg.Ram(w14.params, 0)
    ks = [0, (1 << 14) - 1, 1, 4095, 4096, 12345, 0b10_110_011_101_010, 8191]
    out = {}
    for k in ks:
        addr, = ram.derive_addresses([w14.fu(ram, k)])
        out[k] = got_digits(addr)
        assert np.array_equal(out[k], w14.digits(k)), k
    return out


@pytest.mark.parametrize("K", [2, 3, 8])
def test_batch_equals_single_derivations(w14, singles14, K):
    ram = w14.pkg.Ram(w14.params, 0)
    ks = list(singles14)[:K]
    assert 0 in ks and (1 << 14) - 1 in ks
    fus = [w14.fu(ram, k) for k in ks]
    ram.profile_enable(True)
    ram.profile_reset()
    addrs = ram.derive_addresses(fus)
    prof = ram.profile_get("derive")
    ram.profile_enable(False)
    assert prof["launches"] == 1 and prof["blocks"] == K * 5 * 6, prof
    for k, a in zip(ks, addrs):
        assert np.array_equal(got_digits(a), singles14[k]), (K, k)
    assert ram.roundoff_max() < 0.375


def test_batch_with_a_duplicated_integer(w14, singles14):
    ram = w14.pkg.Ram(w14.params, 0)
    f0, f1 = w14.fu(ram, 12345), w14.fu(ram, 4096)
    addrs = ram.derive_addresses([f0, f1, f0])
    assert len({id(a) for a in addrs}) == 3
    for k, a in zip([12345, 4096, 12345], addrs):
        assert np.array_equal(got_digits(a), singles14[k]), k


# ---- 3. in place --------------------------------------------------------------------------------------------------------------------------
def test_in_place_over_alloc_encrypt_sk_and_derived(w14):
    pkg, o = w14.pkg, w14.o
    ram = pkg.Ram(w14.params, 0)
    k1, k2 = 12345, 4095
    f1, f2 = w14.fu(ram, k1), w14.fu(ram, k2)
    a = pkg.Address.alloc(ram)
    assert ram.derive_addresses([f1], [a])[0] is a
    assert np.array_equal(got_digits(a), w14.digits(k1))
    b = pkg.Address.encrypt_sk(ram, 777, pkg.GLWESecret(ram, w14.sk), o.source(61), o.source(62))
    ram.derive_addresses([f2], [b])
    assert np.array_equal(got_digits(b), w14.digits(k2))
    ram.derive_addresses([f2, f1], [a, b])                                     # both were derived before: overwritten in place
    assert np.array_equal(got_digits(a), w14.digits(k2)) and np.array_equal(got_digits(b), w14.digits(k1))
    c = pkg.Address(w14.params, list(w14.digits(777)))                         # made from host digits (fheram_address_create)
    ram.derive_addresses([f1], [c])
    assert np.array_equal(got_digits(c), w14.digits(k1))


@pytest.mark.parametrize("graph", [0, 1])
def test_read_derive_read_on_one_handle(w14, graph):
    ram = w14.new_ram(0, config={"graph": graph})
    k1, k2 = 12345, 4096
    f1, f2 = w14.fu(ram, k1), w14.fu(ram, k2)
    a, = ram.derive_addresses([f1])
    r1 = ram.read(a, w14.keys).copy()
    ram.derive_addresses([f2], [a])
    r2 = ram.read(a, w14.keys).copy()
    ram.derive_addresses([f1], [a])
    r3 = ram.read(a, w14.keys).copy()                                          # (graph = 1: the third read replays the first one's capture)
    assert np.array_equal(r1, w14.oracle_read(k1)), "first read"
    assert np.array_equal(r2, w14.oracle_read(k2)), "read after the address was overwritten in place"
    assert np.array_equal(r3, r1)
    assert not np.array_equal(r1, r2)


@pytest.mark.parametrize("config", [None, {"memo": 0}], ids=["default", "memo0"])
def test_derive_between_read_prepare_write_and_write(w14, config):
    """stale memo / pre_inv state: the write must not resume from the inverse digits started early for the OLD digits of the handle"""
    pkg = w14.pkg
    k1, k2 = 12345, 4095
    word = np.stack([w14.o.glwe_encrypt_coeff0(0x5A, w14.sk, 71, 72)])
    # the context under test: one handle, overwritten between read_prepare_write and write
    ram = w14.new_ram(0, config=config)
    f1, f2 = w14.fu(ram, k1), w14.fu(ram, k2)
    a, = ram.derive_addresses([f1])
    got_rpw = ram.read_prepare_write(a, w14.keys).copy()
    ram.derive_addresses([f2], [a])
    ram.write(word, a, w14.keys)
    # the comparator: two separately created addresses (host digits) on a second context
    ref = w14.new_ram(0, config=config)
    a1, a2 = pkg.Address(w14.params, list(w14.digits(k1))), pkg.Address(w14.params, list(w14.digits(k2)))
    want_rpw = ref.read_prepare_write(a1, w14.keys).copy()
    ref.write(word, a2, w14.keys)
    assert np.array_equal(got_rpw, want_rpw)
    assert ram.state == ref.state and not ram.state
    assert np.array_equal(ram.store_encrypted(), ref.store_encrypted()), "rows after the write"
    assert np.array_equal(ram.tree(0), ref.tree(0)), "tree after the write"
    assert np.array_equal(ram.read(a, w14.keys), ref.read(a2, w14.keys))


# ---- 4. no wait ---------------------------------------------------------------------------------------------------------------------------
def test_derive_and_read_back_to_back_without_a_sync(w14):
    L = lib()
    ram = w14.new_ram(0)
    ram._use_keys(w14.keys)
    k = 0b10_110_011_101_010
    fu = w14.fu(ram, k)
    a = w14.pkg.Address.alloc(ram)
    fa, aa = (C.c_void_p * 1)(fu._h), (C.c_void_p * 1)(a._device(ram))
    ram.roundoff_reset()
    assert L.fheram_address_derive(ram._h, fa, 1, 0, aa) == ST_OK
    assert L.fheram_read(ram._h, aa[0], None) == ST_OK                         # out = NULL: nothing waits
    out = np.zeros((w14.ws, w14.params.glwe_len()), dtype=np.int64)
    assert L.fheram_result_download(ram._h, out.ctypes.data_as(C.POINTER(C.c_int64))) == ST_OK
    assert np.array_equal(out, w14.oracle_read(k))
    m = C.c_double(-1.0)
    assert L.fheram_roundoff_max(ram._h, C.byref(m)) == ST_OK
    print(f"round-off maximum after derive + read: {m.value}")
    assert 0.0 <= m.value < 0.375


def test_derive_then_read_prepare_write_and_write_without_a_sync(w14):
    """sync; derive(a); read_prepare_write(a); write(a) with no host wait in between: the side-stream work that read_prepare_write starts
    early (the write's inverse digits, read from a's digits) runs behind the derive launch"""
    L = lib()
    word = np.stack([w14.o.glwe_encrypt_coeff0(0x3C, w14.sk, 73, 74)])
    k = 8191
    ram = w14.new_ram(0)
    ram._use_keys(w14.keys)
    fu = w14.fu(ram, k)
    a = w14.pkg.Address.alloc(ram)
    fa, aa = (C.c_void_p * 1)(fu._h), (C.c_void_p * 1)(a._device(ram))
    ram.stage_words(word)
    ram.sync()
    assert L.fheram_address_derive(ram._h, fa, 1, 0, aa) == ST_OK
    assert L.fheram_read_prepare_write(ram._h, aa[0], None) == ST_OK
    assert L.fheram_write(ram._h, None, w14.ws, aa[0]) == ST_OK               # the staged words
    ref = w14.new_ram(0)
    a_ref = w14.pkg.Address(w14.params, list(w14.digits(k)))
    want = ref.read_prepare_write(a_ref, w14.keys).copy()
    ref.write(word, a_ref, w14.keys)
    assert np.array_equal(ram.result(), want)
    assert np.array_equal(ram.store_encrypted(), ref.store_encrypted()), "rows after the write"
    assert np.array_equal(ram.tree(0), ref.tree(0)), "tree after the write"
    assert ram.roundoff_max() < 0.375


# ---- 5. bank ------------------------------------------------------------------------------------------------------------------------------
def test_bank_derive_and_read(w14):
    pkg = w14.pkg
    bank = pkg.RamBank(w14.params, 2, 0)
    for m in range(2):
        bank.load_encrypted(m, w14.rows[m])
    ks = [12345, 4096]
    fus = [pkg.FheUintPrepared.from_host(bank, w14.bits(k)) for k in ks]       # fheram_bank_fheuint_create
    addrs = bank.derive_addresses(fus)
    got = bank.read(addrs, w14.keys).copy()
    shared = bank.read([addrs[1], addrs[1]], w14.keys).copy()                   # one derived handle serves both members
    for m in range(2):
        ram = w14.new_ram(m)
        fu = w14.fu(ram, ks[m])
        old = pkg.Address.set_from_fheuint(ram, fu, sign=False)                # the old entry point on a standalone Ram
        assert np.array_equal(got[m], ram.read(old, w14.keys)), m
        assert np.array_equal(got[m], w14.oracle_read(ks[m], m)), m
        old1 = pkg.Address.set_from_fheuint(ram, w14.fu(ram, ks[1]), sign=False)
        assert np.array_equal(shared[m], ram.read(old1, w14.keys)), ("shared handle", m)
    assert bank.roundoff_max() < 0.375


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(w14):
    pkg, L = w14.pkg, lib()
    ram = w14.new_ram(0)
    ram._use_keys(w14.keys)
    other = pkg.Ram(w14.params, 0)
    bank = pkg.RamBank(w14.params, 2, 0)
    k1, k2 = 12345, 4095
    f1, f2 = w14.fu(ram, k1), w14.fu(ram, k2)
    a, b = ram.derive_addresses([f1, f2])
    before = [got_digits(a), got_digits(b)]
    ha, hb = a._device(ram), b._device(ram)
    foreign_fu, bank_fu = w14.fu(other, k2), pkg.FheUintPrepared.from_host(bank, w14.bits(k2))
    foreign_addr, bank_addr, bank_empty = pkg.Address.alloc(other), pkg.Address.alloc(bank), pkg.Address.alloc(bank)
    narrow = pkg.FheUintPrepared.from_host(ram, w14.bits(k2)[:10])
    VP = C.c_void_p

    def arr(*hs):
        return (VP * len(hs))(*hs)

    def unchanged(what):
        assert np.array_equal(got_digits(a), before[0]) and np.array_equal(got_digits(b), before[1]), what

    def refused(rc, what, needle=None):
        assert rc == ST_INVALID_ARG, (what, rc)
        if needle:
            assert needle in L.fheram_last_error(ram._h).decode(), (what, L.fheram_last_error(ram._h).decode())
        unchanged(what)

    refused(L.fheram_address_derive(ram._h, None, 1, 0, arr(ha)), "null integer list")
    refused(L.fheram_address_derive(ram._h, arr(f2._h), 1, 0, None), "null address list")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, None), 2, 0, arr(ha, hb)), "null integer")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, f2._h), 2, 0, arr(ha, None)), "null address")
    refused(L.fheram_address_derive(ram._h, arr(f2._h), 0, 0, arr(ha)), "n = 0", "FHERAM_DERIVE_MAX")
    refused(L.fheram_address_derive(ram._h, arr(*[f2._h] * 9), 9, 0, arr(*[ha] * 9)), "n = 9", "FHERAM_DERIVE_MAX")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, foreign_fu._h), 2, 0, arr(ha, hb)), "integer of another context", "another context")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, bank_fu._h), 2, 0, arr(ha, hb)), "integer of a bank", "another context")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, f2._h), 2, 0, arr(ha, foreign_addr._device(other))), "address of another context", "another context")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, f2._h), 2, 0, arr(ha, bank_addr._bank(bank))), "address of a bank", "another context")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, narrow._h), 2, 0, arr(ha, hb)), "narrow integer", "the address plan is wider than the encrypted integer")
    refused(L.fheram_address_derive(ram._h, arr(f2._h, f1._h), 2, 0, arr(ha, ha)), "the same address twice", "twice")
    # a null `out` with a live context / bank
    bits10 = np.ascontiguousarray(w14.bits(k2)[:10])
    refused(L.fheram_address_alloc(ram._h, None), "alloc with a null out")
    assert L.fheram_bank_address_alloc(bank._h, None) == ST_INVALID_ARG
    assert L.fheram_bank_fheuint_create(bank._h, bits10.ctypes.data_as(C.POINTER(C.c_int64)), 10, None) == ST_INVALID_ARG
    # the digits of an empty address cannot be downloaded either
    probe = np.zeros((5, w14.params.ggsw_len()), dtype=np.int64)
    blank = pkg.Address.alloc(ram)
    refused(L.fheram_address_download(ram._h, blank._device(ram), probe.ctypes.data_as(C.POINTER(C.c_int64))), "download of an empty address", "empty address")
    with pytest.raises(pkg.FheRamError):
        blank.digits
    # the bank refuses a context's integers and addresses the same way
    assert L.fheram_bank_address_derive(bank._h, arr(f2._h), 1, 0, arr(bank_addr._bank(bank))) == ST_INVALID_ARG
    assert L.fheram_bank_address_derive(bank._h, arr(bank_fu._h), 1, 0, arr(ha)) == ST_INVALID_ARG
    unchanged("bank refusals")
    # an empty address is refused by read (and by the bank's read), by the mirrors too
    empty = pkg.Address.alloc(ram)
    refused(L.fheram_read(ram._h, empty._device(ram), None), "read of an empty address", "empty address")
    refused(L.fheram_read_prepare_write(ram._h, empty._device(ram), None), "read_prepare_write of an empty address", "empty address")
    assert not ram.state
    with pytest.raises(pkg.FheRamError) as e:
        ram.read(empty, w14.keys)
    assert e.value.code == ST_INVALID_ARG and "empty address" in e.value.msg
    for m in range(2):
        bank.load_encrypted(m, w14.rows[m])
    with pytest.raises(pkg.FheRamError) as e:
        bank.read([bank_empty, bank_empty], w14.keys)
    assert e.value.code == ST_INVALID_ARG and "empty address" in e.value.msg
    with pytest.raises(pkg.FheRamError):
        ram.derive_addresses([f1, f2], [a])                                       # the mirrors: list lengths differ
    with pytest.raises(pkg.FheRamError):
        ram.derive_addresses([f1] * 9)
    unchanged("mirror refusals")
    # after all that the context derives and reads correctly
    ram.derive_addresses([f2, f1], [a, empty])
    assert np.array_equal(got_digits(a), w14.digits(k2)) and np.array_equal(got_digits(empty), w14.digits(k1))
    assert np.array_equal(ram.read(empty, w14.keys), w14.oracle_read(k1))
    assert np.array_equal(ram.read(a, w14.keys), w14.oracle_read(k2))
