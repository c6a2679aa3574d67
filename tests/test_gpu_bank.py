"""fheram_bank / RamBank: M RAMs of the same shape under one key set, and read / read_prepare_write / write on a contiguous
range of them as ONE operation (include/fheram.h).

The contract: member m of a bank is int64-identical — every result, every row after a write, tree level 0, the state flag — to a
standalone Ram created with the same parameters and switches, loaded with the same keys and rows and driven through the same
per-member calls; members outside a range are untouched; a refused call changes nothing.  No tolerance anywhere."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from _pkg import load_package

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS = 1, 2, 3, 4
I64P = C.POINTER(C.c_int64)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int64).tobytes()).hexdigest()


def lib():
    return load_package().library()


class World:
    """One key set, n_members encrypted RAMs (different contents) and n_addr encrypted addresses from the oracle's setup side."""

    def __init__(self, po, max_addr, n_members, word_size=4, seed=0, n_addr=3, **crypto):
        pkg = load_package()
        self.pkg, self.po, self.crypto = pkg, po, crypto
        self.max_addr, self.ws, self.M = max_addr, word_size, n_members
        self.o = po.Oracle(po.OParams(max_addr=max_addr, word_size=word_size, **crypto))
        o = self.o
        self.sk = o.secret_gen(1900 + seed)
        self.evk = o.evk_gen(self.sk, 1901 + seed, 1902 + seed)
        self.keys = pkg.EvaluationKeysPrepared.from_dict(self.evk)
        rng = np.random.default_rng(1903 + seed)
        self.data = [rng.integers(0, 256, size=max_addr * word_size, dtype=np.uint8) for _ in range(n_members)]
        self.rows = [o.ram_encrypt(d, self.sk, 1904 + seed + 10 * m, 1905 + seed + 10 * m) for m, d in enumerate(self.data)]
        self.idx = [int(v) for v in rng.integers(0, max_addr, size=n_addr)]
        self.addr_g = [o.address_encrypt(i, self.sk, 2000 + seed + 2 * j, 2001 + seed + 2 * j) for j, i in enumerate(self.idx)]
        self.params = pkg.Parameters(max_addr=max_addr, word_size=word_size, **crypto)
        self.addrs = [pkg.Address(self.params, list(g)) for g in self.addr_g]
        self._okeys = None

    @property
    def okeys(self):
        if self._okeys is None:
            self._okeys = self.o.keys_prepare(self.evk)
        return self._okeys

    def new_bank(self, n_members=None, config=None, load=True):
        n_members = self.M if n_members is None else n_members
        bank = self.pkg.RamBank(self.params, n_members, 0, config=config)
        if load:
            for m in range(n_members):
                bank.load_encrypted(m, self.rows[m])
        return bank

    def new_ram(self, m, config=None):
        ram = self.pkg.Ram(self.params, 0, config=config)
        ram.load_encrypted(self.rows[m])
        return ram

    def new_oram(self, m):
        oram = self.o.ram_new()
        oram.load(self.rows[m])
        return oram

    def words(self, n, seed=0):
        """n words to write: values and their encryptions [n][ws][GLWE]"""
        rng = np.random.default_rng(3000 + seed)
        vals = rng.integers(0, 256, size=(n, self.ws), dtype=np.uint8)
        cts = np.stack([np.stack([self.o.glwe_encrypt_coeff0(int(v), self.sk, 3100 + seed + 16 * k + i, 3500 + seed + 16 * k + i)
                                  for i, v in enumerate(vals[k])]) for k in range(n)])
        return vals, cts

    def check_word(self, cts, data, j, written=False):
        """examples/fhe-ram.rs:104-115: the value, and the noise bound"""
        for i in range(self.ws):
            want = self.o.expected_plain(int(data[i + self.ws * self.idx[j]]), self.o.p.k_glwe_pt, written)
            v, noise = self.o.glwe_decrypt(cts[i], want, self.sk)
            assert v == want, (j, i, v, want, noise)
            assert noise < -(self.o.p.k_glwe_pt + 1), noise


def member_snapshot(bank, m):
    return bank.store_encrypted(m), bank.tree(m, 0), bank.state(m)


def assert_member_is(bank, m, snap, what=""):
    rows, tree, state = snap
    assert bank.state(m) == state, (what, m)
    assert np.array_equal(bank.store_encrypted(m), rows), (what, m)
    assert np.array_equal(bank.tree(m, 0), tree), (what, m)


def assert_member_equals_ram(bank, m, ram, what=""):
    assert bank.state(m) == ram.state, (what, m)
    assert np.array_equal(bank.store_encrypted(m), ram.store_encrypted()), (what, m)
    assert np.array_equal(bank.tree(m, 0), ram.tree(0)), (what, m)


def flow(w, bank, rd, wr, wct):
    """read at rd, read_prepare_write at wr, write wct at wr, read at rd again, on the whole range; everything a host can observe"""
    M = len(rd)
    out = {"read": bank.read([w.addrs[j] for j in rd], w.keys).copy()}
    out["rpw"] = bank.read_prepare_write([w.addrs[j] for j in wr], w.keys).copy()
    out["state_after_rpw"] = [bank.state(m) for m in range(M)]
    out["rows_after_rpw"] = [bank.store_encrypted(m) for m in range(M)]
    out["tree_after_rpw"] = [bank.tree(m, 0) for m in range(M)]
    bank.write(wct, [w.addrs[j] for j in wr], w.keys)
    out["state_after_write"] = [bank.state(m) for m in range(M)]
    out["rows_after_write"] = [bank.store_encrypted(m) for m in range(M)]
    out["tree_after_write"] = [bank.tree(m, 0) for m in range(M)]
    out["readback"] = bank.read([w.addrs[j] for j in wr], w.keys).copy()
    out["result"] = bank.result(0, M).copy()
    return out


def assert_flows_equal(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], list):
            for m, (x, y) in enumerate(zip(a[k], b[k])):
                assert np.array_equal(x, y), (what, k, m)
        else:
            assert np.array_equal(a[k], b[k]), (what, k, np.count_nonzero(np.asarray(a[k]) != np.asarray(b[k])))


RD = [0, 1, 2, 0]   # address of member m for the reads; members 0 and 3 share a handle
WR = [1, 1, 0, 2]   # ... for read_prepare_write / write; members 0 and 1 share a handle


@pytest.fixture(scope="module")
def w14(po):
    return World(po, 1 << 14, 4)


_DEFAULT_FLOW = {}


def default_flow(w, M):
    """the flow on a bank of M members in the default forms, and the words it wrote"""
    if M not in _DEFAULT_FLOW:
        vals, wct = w.words(M, seed=M)
        _DEFAULT_FLOW[M] = (flow(w, w.new_bank(M), RD[:M], WR[:M], wct), vals, wct)
    return _DEFAULT_FLOW[M]


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_bank_equals_standalone_rams_and_oracle_2_14(w14, M):
    w = w14
    got, vals, wct = default_flow(w, M)
    rd, wr = RD[:M], WR[:M]
    assert got["read"].shape == (M, w.ws, w.params.glwe_len())
    assert got["state_after_rpw"] == [True] * M and got["state_after_write"] == [False] * M
    assert np.array_equal(got["result"], got["readback"])
    for m in range(M):
        ram, oram = w.new_ram(m), w.new_oram(m)
        a_rd, a_wr = w.addrs[rd[m]], w.addrs[wr[m]]
        o_rd, o_wr = w.o.address_new(w.addr_g[rd[m]]), w.o.address_new(w.addr_g[wr[m]])
        r = ram.read(a_rd, w.keys)
        assert np.array_equal(got["read"][m], r), (M, m, np.count_nonzero(got["read"][m] != r))
        assert np.array_equal(r, oram.read(o_rd, w.okeys)), (M, m)
        w.check_word(got["read"][m], w.data[m], rd[m])
        r = ram.read_prepare_write(a_wr, w.keys)
        assert np.array_equal(got["rpw"][m], r), (M, m, np.count_nonzero(got["rpw"][m] != r))
        assert np.array_equal(r, oram.read_prepare_write(o_wr, w.okeys)), (M, m)
        assert ram.state is True
        assert np.array_equal(got["rows_after_rpw"][m], ram.store_encrypted()), (M, m)
        assert np.array_equal(got["tree_after_rpw"][m], ram.tree(0)), (M, m)
        assert np.array_equal(got["tree_after_rpw"][m], oram.tree(0)), (M, m)
        ram.write(wct[m], a_wr, w.keys)
        oram.write(wct[m], o_wr, w.okeys)
        assert ram.state is False
        assert np.array_equal(got["rows_after_write"][m], ram.store_encrypted()), (M, m)
        assert np.array_equal(got["rows_after_write"][m], oram.store()), (M, m)
        assert np.array_equal(got["tree_after_write"][m], ram.tree(0)), (M, m)
        assert np.array_equal(got["tree_after_write"][m], oram.tree(0)), (M, m)
        r = ram.read(a_wr, w.keys)
        assert np.array_equal(got["readback"][m], r), (M, m, np.count_nonzero(got["readback"][m] != r))
        assert np.array_equal(r, oram.read(o_wr, w.okeys)), (M, m)
        data2 = w.data[m].copy()
        data2[w.ws * w.idx[wr[m]]: w.ws * (w.idx[wr[m]] + 1)] = vals[m]
        w.check_word(got["readback"][m], data2, wr[m], written=True)


def test_ranges_and_mixed_state_2_14(w14):
    w = w14
    pkg = load_package()
    M = 4
    bank = w.new_bank(M)
    rams = [w.new_ram(m) for m in range(M)]
    A = [w.addrs[j] for j in WR]
    vals, wct = w.words(M, seed=40)

    def outside(first, n):
        return {m: member_snapshot(bank, m) for m in range(M) if not first <= m < first + n}

    def check_outside(snaps, what):
        for m, s in snaps.items():
            assert_member_is(bank, m, s, what)

    # read_prepare_write on [1, 3)
    snaps = outside(1, 2)
    got = bank.read_prepare_write(A[1:3], w.keys, first=1)
    check_outside(snaps, "rpw [1,3)")
    for k, m in enumerate((1, 2)):
        assert np.array_equal(got[k], rams[m].read_prepare_write(A[m], w.keys)), m
        assert_member_equals_ram(bank, m, rams[m], "rpw [1,3)")
    assert [bank.state(m) for m in range(M)] == [False, True, True, False]
    # reads on [0, 1) and [3, 4) while members 1 and 2 sit between read_prepare_write and write
    for m in (0, 3):
        snaps = outside(m, 1)
        got = bank.read([w.addrs[RD[m]]], w.keys, first=m)
        check_outside(snaps, f"read [{m},{m + 1})")
        assert np.array_equal(got[0], rams[m].read(w.addrs[RD[m]], w.keys)), m
        assert_member_equals_ram(bank, m, rams[m], "single read")
    # a read on the whole bank is refused, and nothing is changed
    snaps = outside(0, 0)
    with pytest.raises(pkg.FheRamError) as e:
        bank.read(A, w.keys)
    assert e.value.code == ST_STATE and "member 1" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:
        bank.read_prepare_write(A, w.keys)
    assert e.value.code == ST_STATE
    check_outside(snaps, "refused read")
    # a write on the whole bank is refused (members 0 and 3 are not prepared)
    with pytest.raises(pkg.FheRamError) as e:
        bank.write(wct, A, w.keys)
    assert e.value.code == ST_STATE and "member 0" in e.value.msg
    check_outside(snaps, "refused write")
    # write on [1, 3)
    snaps = outside(1, 2)
    bank.write(wct[1:3], A[1:3], w.keys, first=1)
    check_outside(snaps, "write [1,3)")
    for m in (1, 2):
        rams[m].write(wct[m], A[m], w.keys)
        assert_member_equals_ram(bank, m, rams[m], "write [1,3)")
    assert [bank.state(m) for m in range(M)] == [False] * M
    # single-member read_prepare_write / write (the plain operation, memo included) between ranges, then the whole bank again
    got = bank.read_prepare_write([A[3]], w.keys, first=3)
    assert np.array_equal(got[0], rams[3].read_prepare_write(A[3], w.keys))
    got = bank.read(A[:3], w.keys, first=0)
    for m in range(3):
        assert np.array_equal(got[m], rams[m].read(A[m], w.keys)), m
    bank.write(wct[3:4], [A[3]], w.keys, first=3)
    rams[3].write(wct[3], A[3], w.keys)
    got = bank.read(A, w.keys)
    for m in range(M):
        assert np.array_equal(got[m], rams[m].read(A[m], w.keys)), m
        assert_member_equals_ram(bank, m, rams[m], "end")
    # two read_prepare_write ranges, one write over both
    bank.read_prepare_write(A[:2], w.keys, first=0)
    bank.read_prepare_write(A[2:], w.keys, first=2)
    bank.write(wct[::-1].copy(), A, w.keys)
    for m in range(M):
        rams[m].read_prepare_write(A[m], w.keys)
        rams[m].write(wct[M - 1 - m], A[m], w.keys)
        assert_member_equals_ram(bank, m, rams[m], "two ranges, one write")


FORMS = [{"tail": 0}, {"tail_ep": 0}, {"mid": 0}, {"fuse": 0}, {"chain_y": 0}, {"memo": 0}, {"pre_inv": 0}, {"safe": 1}, {"graph": 1},
         {"tail_test": 1}, {"tail_test": 2}, {"mid_test": 1}]


@pytest.mark.parametrize("config", FORMS, ids=["-".join(f"{k}{v}" for k, v in c.items()) for c in FORMS])
@pytest.mark.parametrize("M", [2, 3])
def test_forced_forms_equal_the_default_form_2_14(w14, M, config):
    w = w14
    want, vals, wct = default_flow(w, M)
    got = flow(w, w.new_bank(M, config=config), RD[:M], WR[:M], wct)
    assert_flows_equal(got, want, (M, config))


@pytest.fixture(scope="module", params=["source", "readme"])
def w16(po, request):
    """2^16: 16 rows, coordinate 1 has two digits (base2d [[3,3,3,3],[3,1]]).  "readme": the 5-limb trace keys (the <5, ...> instantiations)."""
    crypto = {} if request.param == "source" else {"k_glwe_pt": 9, "k_evk_trace": 85}
    return World(po, 1 << 16, 4, seed=80, n_addr=3, **crypto)


def profiled(bank, fn, classes):
    bank.profile_enable(True)
    bank.profile_reset()
    out = fn()
    prof = {c: bank.profile_get(c) for c in classes}
    bank.profile_enable(False)
    return out, prof


CLASSES = ["write_chain_launch", "read_chain_launch", "keyswitch_tail_launch", "keyswitch_mid_launch", "ext_product_mid_launch"]


def test_table_kernels_run_2_16(w16):
    """M = 2 at ws = 4 is 8 ciphertexts = TAIL_GROUPS: the rows' chains of both members are ONE k_read_chain_t / k_write_chain_t launch
    and the end of a read ONE k_trace_tail_t.  A bank that ran everything per member would show two launches of each."""
    w = w16
    M = 2
    rows = w.params.rows()
    bank = w.new_bank(M)
    rams = [w.new_ram(m) for m in range(M)]
    A = [w.addrs[j] for j in WR[:M]]
    vals, wct = w.words(M, seed=16)
    t0 = bank.tail_stats()
    got, prof = profiled(bank, lambda: bank.read(A, w.keys), CLASSES)
    assert prof["keyswitch_tail_launch"]["launches"] == 1 and prof["keyswitch_tail_launch"]["blocks"] == M * w.ws * 12, prof
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * M * w.ws, prof
    for m in range(M):
        assert np.array_equal(got[m], rams[m].read(A[m], w.keys)), m
        w.check_word(got[m], w.data[m], WR[m])
    got, prof = profiled(bank, lambda: bank.read_prepare_write(A, w.keys), CLASSES)
    assert prof["keyswitch_tail_launch"]["launches"] == 1 and prof["read_chain_launch"]["launches"] == 1, prof
    for m in range(M):
        assert np.array_equal(got[m], rams[m].read_prepare_write(A[m], w.keys)), m
        assert_member_equals_ram(bank, m, rams[m], "rpw")
    _, prof = profiled(bank, lambda: bank.write(wct, A, w.keys), CLASSES)
    assert prof["write_chain_launch"]["launches"] == 1 and prof["write_chain_launch"]["blocks"] == rows * M * w.ws, prof
    for m in range(M):
        rams[m].write(wct[m], A[m], w.keys)
        assert_member_equals_ram(bank, m, rams[m], "write")
    got = bank.read(A, w.keys)
    for m in range(M):
        assert np.array_equal(got[m], rams[m].read(A[m], w.keys)), m
        data2 = w.data[m].copy()
        data2[w.ws * w.idx[WR[m]]: w.ws * (w.idx[WR[m]] + 1)] = vals[m]
        w.check_word(got[m], data2, WR[m], written=True)
    t1 = bank.tail_stats()
    assert t1["launches"] > t0["launches"] and t1["fallbacks"] == t0["fallbacks"], (t0, t1)


@pytest.mark.parametrize("M", [3, 4])
def test_wider_banks_end_in_the_mid_chain_2_16(w16, M):
    """12 and 16 ciphertexts: the end of a read is k_chain_mid over the whole range — no tail launch, in particular none per member"""
    w = w16
    rows = w.params.rows()
    bank = w.new_bank(M)
    A = [w.addrs[j] for j in WR[:M]]
    vals, wct = w.words(M, seed=60 + M)
    t0 = bank.tail_stats()
    got, prof = profiled(bank, lambda: bank.read(A, w.keys), CLASSES)
    assert prof["keyswitch_mid_launch"]["launches"] >= 1 and prof["keyswitch_tail_launch"]["launches"] == 0, prof
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * M * w.ws, prof
    rams = [w.new_ram(m) for m in range(M)]
    for m in range(M):
        assert np.array_equal(got[m], rams[m].read(A[m], w.keys)), m
    got = bank.read_prepare_write(A, w.keys)
    _, prof = profiled(bank, lambda: bank.write(wct, A, w.keys), CLASSES)
    assert prof["write_chain_launch"]["launches"] == 1 and prof["write_chain_launch"]["blocks"] == rows * M * w.ws, prof
    assert prof["keyswitch_tail_launch"]["launches"] == 0, prof
    for m in range(M):
        assert np.array_equal(got[m], rams[m].read_prepare_write(A[m], w.keys)), m
        rams[m].write(wct[m], A[m], w.keys)
        assert_member_equals_ram(bank, m, rams[m], "write")
    assert bank.tail_stats()["launches"] == t0["launches"]
    ms = bank.mid_stats()
    assert ms["launches"] > 0 and ms["fallbacks"] == 0, ms


@pytest.fixture(scope="module")
def w16x8(po):
    """2^16 at word size 1, eight members: 16 rows each, 128 ciphertext rows in all"""
    return World(po, 1 << 16, 8, word_size=1, seed=120, n_addr=3)


@pytest.mark.parametrize("first,n", [(0, 8), (3, 5)], ids=["all-8", "members-3-to-7"])
def test_eight_members_one_row_chain_2_16(w16x8, first, n):
    """The smallest shape where a range's row chain is the fused launch with source-map entries 4..7 in use: 16 rows x 8 members, and
    the sub-range [3, 8) of it (80 ciphertext rows, the identity map relative to the range's view).  read, read_prepare_write, write
    and the read-back are each ONE read_chain_launch / write_chain_launch of rows * n blocks; every member of the range equals its
    standalone Ram, every member outside it is untouched."""
    w = w16x8
    M, rows = 8, w.params.rows()
    bank = w.new_bank(M)
    rams = [w.new_ram(first + k) for k in range(n)]
    outside = {m: member_snapshot(bank, m) for m in range(M) if not first <= m < first + n}
    RDj = [(first + k) % 3 for k in range(n)]
    WRj = [(2 * (first + k) + 1) % 3 for k in range(n)]
    RDa, WRa = [w.addrs[j] for j in RDj], [w.addrs[j] for j in WRj]
    vals, wct = w.words(n, seed=200 + first)

    def one_chain(prof, cls):
        assert prof[cls]["launches"] == 1 and prof[cls]["blocks"] == rows * n * w.ws, (cls, prof)

    got, prof = profiled(bank, lambda: bank.read(RDa, w.keys, first=first), CLASSES)
    one_chain(prof, "read_chain_launch")
    for k in range(n):
        assert np.array_equal(got[k], rams[k].read(RDa[k], w.keys)), k
        w.check_word(got[k], w.data[first + k], RDj[k])
    got, prof = profiled(bank, lambda: bank.read_prepare_write(WRa, w.keys, first=first), CLASSES)
    one_chain(prof, "read_chain_launch")
    for k in range(n):
        assert np.array_equal(got[k], rams[k].read_prepare_write(WRa[k], w.keys)), k
        assert_member_equals_ram(bank, first + k, rams[k], "rpw")
    _, prof = profiled(bank, lambda: bank.write(wct, WRa, w.keys, first=first), CLASSES)
    one_chain(prof, "write_chain_launch")
    for k in range(n):
        rams[k].write(wct[k], WRa[k], w.keys)
        assert_member_equals_ram(bank, first + k, rams[k], "write")
    got, prof = profiled(bank, lambda: bank.read(WRa, w.keys, first=first), CLASSES)
    one_chain(prof, "read_chain_launch")
    for k in range(n):
        assert np.array_equal(got[k], rams[k].read(WRa[k], w.keys)), k
        data2 = w.data[first + k].copy()
        data2[w.ws * w.idx[WRj[k]]: w.ws * (w.idx[WRj[k]] + 1)] = vals[k]
        w.check_word(got[k], data2, WRj[k], written=True)
    for m, snap in outside.items():
        assert_member_is(bank, m, snap, "outside the range")


def test_tail_fallback_with_per_member_operands_2_16(w16):
    """tail_test: the bank's k_trace_tail_t gives up late and the predicated k_read_chain_t behind it redoes coordinate 1's products
    (operands of member y / ws) and the trace from the packed rows"""
    w = w16
    M = 2
    bank = w.new_bank(M, config={"tail_test": 1})
    ref = w.new_bank(M)
    A = [w.addrs[j] for j in WR[:M]]
    vals, wct = w.words(M, seed=17)
    t0 = bank.tail_stats()
    got = bank.read(A, w.keys)
    t1 = bank.tail_stats()
    assert t1["launches"] == t0["launches"] + 1 and t1["fallbacks"] == t0["fallbacks"] + 1, (t0, t1)
    assert np.array_equal(got, ref.read(A, w.keys))
    got = bank.read_prepare_write(A, w.keys)
    t2 = bank.tail_stats()
    assert t2["fallbacks"] > t1["fallbacks"], (t1, t2)
    assert np.array_equal(got, ref.read_prepare_write(A, w.keys))
    bank.write(wct, A, w.keys)
    ref.write(wct, A, w.keys)
    for m in range(M):
        assert_member_is(bank, m, member_snapshot(ref, m), "write behind a tail that gave up")


def test_one_row_and_identical_members_2_12(po):
    """2^12: one row per sub-RAM, one coordinate (n2 == 1).  Members with the same rows, the same address and the same words stay
    identical to each other and to the standalone context."""
    w = World(po, 1 << 12, 1, seed=50, n_addr=2)
    pkg = load_package()
    M = 3
    bank = pkg.RamBank(w.params, M)
    for m in range(M):
        bank.load_encrypted(m, w.rows[0])
    ram = w.new_ram(0)
    a, b = w.addrs
    vals, wct = w.words(1, seed=12)
    got = bank.read([a] * M, w.keys)
    want = ram.read(a, w.keys)
    for m in range(M):
        assert np.array_equal(got[m], want), m
    w.check_word(got[0], w.data[0], 0)
    got = bank.read_prepare_write([b] * M, w.keys)
    want = ram.read_prepare_write(b, w.keys)
    for m in range(M):
        assert np.array_equal(got[m], want), m
    bank.write(np.concatenate([wct] * M), [b] * M, w.keys)
    ram.write(wct[0], b, w.keys)
    rows = ram.store_encrypted()
    for m in range(M):
        assert np.array_equal(bank.store_encrypted(m), rows), m
        assert bank.state(m) is False
    got = bank.read([b] * M, w.keys)
    want = ram.read(b, w.keys)
    data2 = w.data[0].copy()
    data2[w.ws * w.idx[1]: w.ws * (w.idx[1] + 1)] = vals[0]
    for m in range(M):
        assert np.array_equal(got[m], want), m
    w.check_word(got[M - 1], data2, 1, written=True)
    with pytest.raises(pkg.FheRamError) as e:     # no tree at one coordinate, as for a context
        bank.tree(0, 0)
    assert e.value.code == ST_INVALID_ARG


def test_one_row_ranges_of_distinct_members_2_12(po):
    """2^12 again, where the rows themselves are the tree top and part / tmp stand in for the arenas — now with a word size of 2, so
    that a member's offset is not its ciphertext's, distinct members, and ranges that start behind member 0: every member equals its
    standalone Ram and the members outside a range keep their rows and state."""
    M = 3
    w = World(po, 1 << 12, M, word_size=2, seed=120, n_addr=2)
    bank = w.new_bank(M)
    rams = [w.new_ram(m) for m in range(M)]
    a, b = w.addrs
    vals, wct = w.words(M, seed=121)

    def member0_untouched(what):   # (no tree at one coordinate: rows and state are all a member has)
        assert bank.state(0) is False, what
        assert np.array_equal(bank.store_encrypted(0), rows0), what

    rows0 = bank.store_encrypted(0)
    got = bank.read_prepare_write([a, b], w.keys, first=1)
    for k, (m, adr) in enumerate(((1, a), (2, b))):
        assert np.array_equal(got[k], rams[m].read_prepare_write(adr, w.keys)), m
        assert bank.state(m) is True
    member0_untouched("rpw [1,3)")
    bank.write(wct[1:3], [a, b], w.keys, first=1)
    for m, adr in ((1, a), (2, b)):
        rams[m].write(wct[m], adr, w.keys)
        assert np.array_equal(bank.store_encrypted(m), rams[m].store_encrypted()), m
        assert bank.state(m) is False
    member0_untouched("write [1,3)")
    got = bank.read([a], w.keys, first=2)
    assert np.array_equal(got[0], rams[2].read(a, w.keys))
    res = bank.result(1, 2)   # member 1: what its read_prepare_write left (in another buffer); member 2: the read just done
    assert np.array_equal(res[0], rams[1].result()) and np.array_equal(res[1], rams[2].result())
    got = bank.read([b, a, b], w.keys)
    for m, adr in enumerate((b, a, b)):
        assert np.array_equal(got[m], rams[m].read(adr, w.keys)), m
    data1 = w.data[1].copy()
    data1[w.ws * w.idx[0]: w.ws * (w.idx[0] + 1)] = vals[1]
    w.check_word(got[1], data1, 0, written=True)
    w.check_word(got[0], w.data[0], 1)
    member0_untouched("end")


def test_2_18_two_members_against_two_contexts():
    """Synthetic normalised limbs for keys, address digits, rows and words (no oracle encryption at this size): a bank step equals two
    standalone contexts by SHA-256 of results and rows, takes no fallback, and its round-off stays where the contexts' own is."""
    pkg = load_package()
    M, ws, max_addr, n = 2, 4, 1 << 18, 4096
    p = pkg.Parameters(max_addr=max_addr, word_size=ws)
    rng = np.random.default_rng(1234)

    def synth(shape):
        return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)

    keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth((12, 3 * 4 * 2 * n))), synth(4 * 5 * 2 * n), synth(4 * 5 * 2 * n))
    n_digits = p.base2d().as_1d().size()
    addrs = [pkg.Address(p, list(synth((n_digits, p.ggsw_len())))) for _ in range(M)]
    rows = [synth((ws, p.rows(), p.glwe_len())) for _ in range(M)]
    words = synth((M, ws, p.glwe_len()))
    bank = pkg.RamBank(p, M)
    rams = [pkg.Ram(p, 0) for _ in range(M)]
    for m in range(M):
        bank.load_encrypted(m, rows[m])
        rams[m].load_encrypted(rows[m])
    got = {"read": bank.read(addrs, keys).copy(), "rpw": bank.read_prepare_write(addrs, keys).copy()}
    bank.write(words, addrs, keys)
    for m in range(M):
        assert sha(got["read"][m]) == sha(rams[m].read(addrs[m], keys)), m
        assert sha(got["rpw"][m]) == sha(rams[m].read_prepare_write(addrs[m], keys)), m
        rams[m].write(words[m], addrs[m], keys)
        assert sha(bank.store_encrypted(m)) == sha(rams[m].store_encrypted()), m
        assert sha(bank.tree(m, 0)) == sha(rams[m].tree(0)), m
        assert bank.state(m) is False
    t, md = bank.tail_stats(), bank.mid_stats()
    assert t["launches"] > 0 and t["fallbacks"] == 0, t
    assert md["fallbacks"] == 0, md
    ro_bank = bank.roundoff_max()
    ro_ctx = max(r.roundoff_max() for r in rams)
    print(f"roundoff_max: bank {ro_bank:.6f}, standalone contexts {ro_ctx:.6f}")
    assert ro_bank < 3 / 8
    assert ro_ctx / 2 <= ro_bank <= ro_ctx * 2, (ro_bank, ro_ctx)


def test_refused_calls_change_nothing(w14):
    w = w14
    pkg = load_package()
    L = lib()
    M = 3
    bank = w.new_bank(M)
    bank.read([w.addrs[0]] * M, w.keys)   # (loads the keys)
    A = [w.addrs[j] for j in WR[:M]]
    h = [a._bank(bank) for a in A]
    vals, wct = w.words(M, seed=70)
    snaps = [member_snapshot(bank, m) for m in range(M)]
    out = np.zeros((M, w.ws, w.params.glwe_len()), dtype=np.int64)

    def c_op(fn, first, n, handles, buf=None, on=None):
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        return fn((on or bank)._h, first, n, arr, buf.ctypes.data_as(I64P) if buf is not None else None)

    def c_write(first, n, handles, words):
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        return L.fheram_bank_write(bank._h, first, n, words.ctypes.data_as(I64P) if words is not None else None, arr)

    def unchanged(what):
        assert L.fheram_bank_last_error(bank._h), what
        for m in range(M):
            assert_member_is(bank, m, snaps[m], what)

    for fn in (L.fheram_bank_read, L.fheram_bank_read_prepare_write):
        for first, n in ((-1, 2), (2, 2), (0, 0), (0, M + 1), (M, 1)):
            assert c_op(fn, first, n, h, out) == ST_INVALID_ARG, (first, n)
            assert b"range" in L.fheram_bank_last_error(bank._h)
        assert c_op(fn, 0, 2, [h[0], None], out) == ST_INVALID_ARG
        assert fn(bank._h, 0, 2, None, None) == ST_INVALID_ARG
        unchanged("range / null")
    other_bank = w.new_bank(2)
    other_ram = w.new_ram(0)
    for foreign in (w.addrs[0]._bank(other_bank), w.addrs[0]._device(other_ram)):
        assert c_op(L.fheram_bank_read, 0, 2, [h[0], foreign], out) == ST_INVALID_ARG
        assert b"does not belong" in L.fheram_bank_last_error(bank._h)
        assert c_op(L.fheram_bank_read_prepare_write, 1, 2, [foreign, h[1]], out) == ST_INVALID_ARG
    unchanged("foreign address")
    # the Python layer refuses the same calls
    for bad in (lambda: bank.read(A, w.keys, first=1), lambda: bank.read([], w.keys), lambda: bank.read(A[:1], w.keys, first=-1),
                lambda: bank.read([A[0], None], w.keys), lambda: bank.result(2, 2), lambda: bank.store_encrypted(M)):
        with pytest.raises(pkg.FheRamError) as e:
            bad()
        assert e.value.code == ST_INVALID_ARG
    unchanged("python layer")
    # keys missing; a member never uploaded
    nokeys = w.new_bank(2)
    assert c_op(L.fheram_bank_read, 0, 2, [a._bank(nokeys) for a in A[:2]], out, on=nokeys) == ST_KEYS
    assert b"keys" in L.fheram_bank_last_error(nokeys._h)
    partial = w.new_bank(3, load=False)
    partial.load_encrypted(0, w.rows[0])
    partial.load_encrypted(2, w.rows[2])
    with pytest.raises(pkg.FheRamError) as e:
        partial.read(A, w.keys)
    assert e.value.code == ST_UNINITIALIZED and "member 1" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:
        partial.store_encrypted(1)
    assert e.value.code == ST_UNINITIALIZED
    assert np.array_equal(partial.read([A[2]], w.keys, first=2)[0], bank.read([A[2]], w.keys, first=2)[0])   # its loaded members work
    # write: state, wrong word count, null words, foreign address
    assert c_write(0, M, h, wct) == ST_STATE
    unchanged("write without read_prepare_write")
    bank.read_prepare_write(A, w.keys)
    snaps = [member_snapshot(bank, m) for m in range(M)]
    with pytest.raises(pkg.FheRamError) as e:
        bank.write(wct[:2], A, w.keys)
    assert e.value.code == ST_INVALID_ARG and "ram.rs:243" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:
        bank.write(wct[:, :2], A, w.keys)
    assert e.value.code == ST_INVALID_ARG
    assert c_write(0, M, h, None) == ST_INVALID_ARG
    assert c_write(0, M + 1, h, wct) == ST_INVALID_ARG
    assert c_write(0, M, [h[0], w.addrs[0]._bank(other_bank), h[2]], wct) == ST_INVALID_ARG
    assert c_op(L.fheram_bank_read, 0, 1, h[:1], out) == ST_STATE
    unchanged("refused writes")
    # the bank that refused all of these still works, and equals one that was never misused
    bank.write(wct, A, w.keys)
    clean = w.new_bank(M)
    clean.read_prepare_write(A, w.keys)
    clean.write(wct, A, w.keys)
    for m in range(M):
        assert_member_is(bank, m, member_snapshot(clean, m), "after the refusals")
