"""fheram_bank_select / fheram_bank_selector_* / fheram_bank_write_list_selected (RamBank.select, .selector, .derive_selectors,
.write_list_selected): pick one of m candidate words by an ENCRYPTED index on the device, and write what was picked (include/fheram.h).

The contract, in the oracle's own operations: for a selector of b bits and m <= 2^b candidates, per word ciphertext y,
    packed_y = glwe_normalize(sum_j glwe_rotate(j, c_j[y]))
    out[y]   = ORam(OParams(max_addr = 2^b)).load(packed).read(address_new(selector digits))
and the selector digits are address_from_fheuint(bits[f : f + b], sign=False) of an oracle with max_addr = 2^b.
Every comparison is np.array_equal on int64; the noise of a decrypted output is printed, not bounded (DESIGN.md 14 records it).
Banks are at max_addr = 2^12 (one row, one coordinate) unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import World, lib, sha

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS, ST_RANGE, ST_DEVICE = 1, 2, 3, 4, 6, 7
VALUE = 0xB5E3A6D9   # the encrypted integer selectors are derived from: every field used below has set and clear bits
N_BITS = 32


class SelWorld(World):
    """a World plus what a select needs of the oracle: small oracles of max_addr = 2^b, encrypted integers, selector digits"""

    def __init__(self, po, max_addr, n_members, word_size, seed, **crypto):
        super().__init__(po, max_addr, n_members, word_size=word_size, seed=seed, n_addr=3, **crypto)
        self._small, self._ints, self._digits, self._cand = {}, {}, {}, {}

    def oparams(self, max_addr, **over):
        """OParams of another shape under this world's crypto block (its keys have that block's limb counts); `over` wins"""
        return self.po.OParams(**{**self.crypto, "max_addr": max_addr, "word_size": self.ws, **over})

    def small(self, b):
        """(oracle of max_addr = 2^b with this world's word size and crypto block, its prepared keys)"""
        if b not in self._small:
            ob = self.po.Oracle(self.oparams(1 << b))
            self._small[b] = (ob, ob.keys_prepare(self.evk))
        return self._small[b]

    def bits(self, value):
        if value not in self._ints:
            self._ints[value] = self.o.fheuint_encrypt(value, N_BITS, self.sk, 5200 + value % 997, 5201 + value % 997)
        return self._ints[value]

    def digits(self, value, f, b):
        """the selector of bits [f, f + b) of `value`: [n_digits][ggsw_len]"""
        if (value, f, b) not in self._digits:
            self._digits[(value, f, b)] = self.small(b)[0].address_from_fheuint(self.bits(value)[f:f + b], sign=False)
        return self._digits[(value, f, b)]

    def index_digits(self, idx, b):
        return self.digits(idx, 0, b)

    def candidates(self, m, seed=40):
        """m words [m][ws][GLWE] with their values [m][ws]"""
        if (m, seed) not in self._cand:
            self._cand[(m, seed)] = self.words(m, seed=seed)
        return self._cand[(m, seed)]

    def oselect(self, b, cands, digits):
        """the contract: cands [m][ws][GLWE] int64 -> [ws][GLWE]"""
        ob, okeys = self.small(b)
        cands = np.asarray(cands, dtype=np.int64)
        packed = np.stack([ob.glwe_normalize(sum(ob.glwe_rotate(j, cands[j][y]) for j in range(cands.shape[0]))) for y in range(self.ws)])
        oram = ob.ram_new()
        oram.load(packed.reshape(self.ws, 1, -1))
        return oram.read(ob.address_new(digits), okeys)

    def selector(self, bank, idx, b):
        return self.pkg.Selector.from_digits(bank, b, list(self.index_digits(idx, b)))

    def check_value(self, cts, values, what=""):
        """cts [ws][GLWE] decrypt to `values` [ws] (None: 0); returns the largest log2 noise"""
        worst = -1e9
        for i in range(self.ws):
            want = 0 if values is None else self.o.expected_plain(int(values[i]), self.o.p.k_glwe_pt, True)
            v, noise = self.o.glwe_decrypt(cts[i], want, self.sk)
            assert v == want, (what, i, v, want, noise)
            worst = max(worst, noise)
        return worst


@pytest.fixture(scope="module")
def w2(po):
    return SelWorld(po, 1 << 12, 3, 2, seed=300)


@pytest.fixture(scope="module")
def w1(po):
    return SelWorld(po, 1 << 12, 1, 1, seed=310)


@pytest.fixture(scope="module")
def w13(po):
    return SelWorld(po, 1 << 13, 3, 2, seed=320)


@pytest.fixture(scope="module")
def bank2(w2):
    """one default bank of three members (word size 2) shared by the tests that change no member"""
    bank = w2.new_bank(3)
    bank._use_keys(w2.keys)
    return bank


def host_srcs(pkg, m, first=0):
    return [pkg.Src.host(first + j) for j in range(m)]


# ---- 1. selectors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 4, 5])
def test_selector_digits_equal_the_oracle(w1, b):
    """b = 4 is the plan [3, 1] (lsh restarts at the second digit's own offset), b = 5 is [3, 2]; first_bit 0, 7 and 32 - b in ONE call from ONE
    integer (three launches: three distinct (first_bit, bits) pairs)"""
    w, pkg = w1, w1.pkg
    bank = w.new_bank(1)
    assert w.small(b)[0].n_digits == {1: 1, 3: 1, 4: 2, 5: 2}[b]
    fu = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))
    firsts = [0, 7, N_BITS - b]
    sels = [bank.selector(b) for _ in firsts]
    assert all(s.n_digits() == w.small(b)[0].n_digits for s in sels)
    bank.profile_enable(True)
    bank.derive_selectors([fu] * 3, firsts, sels)
    bank.sync()
    prof = bank.profile_get("derive")
    assert prof["launches"] == 3 and prof["blocks"] == 3 * 6 * sels[0].n_digits(), prof
    bank.profile_enable(False)
    for f, s in zip(firsts, sels):
        assert np.array_equal(s.download(), w.digits(VALUE, f, b)), (b, f)
    # in place: over an earlier derivation, and over host digits (fheram_bank_selector_create)
    other = VALUE ^ 0xFFFFFFFF
    fu2 = pkg.FheUintPrepared.from_host(bank, w.bits(other))
    made = pkg.Selector.from_digits(bank, b, list(w.digits(VALUE, 0, b)))
    assert np.array_equal(made.download(), w.digits(VALUE, 0, b))
    bank.derive_selectors([fu2, fu2], [7, 7], [sels[0], made])   # one launch: one (first_bit, bits) pair
    assert np.array_equal(sels[0].download(), w.digits(other, 7, b)), b
    assert np.array_equal(made.download(), w.digits(other, 7, b)), b
    assert np.array_equal(sels[1].download(), w.digits(VALUE, 7, b)), "a selector that was not named changed"


# ---- 2. select against the oracle ---------------------------------------------------------------------------------------------------------
SHAPES = [(1, 2), (2, 3), (3, 8), (5, 20)]   # (bits, candidates): 3 is no power of two, 20 has two digits
_SINGLE = {}


def indices(b, m):
    return sorted({0, m // 2, m - 1} | ({m} if m < (1 << b) else set()))   # also one index >= m where there is one: decrypts to 0


def single(w, bank, b, m, idx):
    """select of candidates(m) at idx on the default bank, computed once: (output, oracle output)"""
    key = (id(w), b, m, idx)
    if key not in _SINGLE:
        vals, cts = w.candidates(m)
        got = bank.select([w.selector(bank, idx, b)], [host_srcs(w.pkg, m)], host_words=cts)
        _SINGLE[key] = (got[0].copy(), w.oselect(b, cts, w.index_digits(idx, b)))
    return _SINGLE[key]


@pytest.mark.parametrize("b,m", SHAPES)
def test_select_equals_the_oracle_and_decrypts(w2, bank2, b, m):
    w = w2
    vals, cts = w.candidates(m)
    for idx in indices(b, m):
        got, want = single(w, bank2, b, m, idx)
        assert got.shape == (w.ws, w.params.glwe_len())
        assert np.array_equal(got, want), (b, m, idx, np.count_nonzero(got != want))
        noise = w.check_value(got, vals[idx] if idx < m else None, (b, m, idx))
        print(f"select b={b} m={m} idx={idx}: log2 noise {noise:.2f}")
    last = indices(b, m)[-1]
    again = bank2.select([w.selector(bank2, last, b)], [host_srcs(w.pkg, m)], host_words=cts, download=False)
    assert again is None
    assert np.array_equal(bank2.select_result(0, 1)[0], single(w, bank2, b, m, last)[0]), "select_result after download=False"


# ---- 3. every source kind ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [None, {"memo": 0}], ids=["memo", "memo0"])
def test_every_source_kind(w2, config):
    """candidates from: a member's read result (d_res), a member's read_prepare_write result (kept in d_trtop under memo), entries of a read list with a
    repeated member, the previous select's output, ZERO and host words — eight selects (n * ws = 16) over the same eight candidates in one call;
    afterwards the prepared member resumes its write exactly as a bank that ran no select"""
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    vals, cts = w.candidates(4, seed=41)
    a = w.addrs

    def prepare(bank):
        r0 = bank.read([a[0]], w.keys, first=0)[0]
        r1 = bank.read_prepare_write([a[1]], w.keys, first=1)[0]
        lst = bank.read_list([2, 0, 2], [a[2], a[1], a[0]], w.keys)
        return r0, r1, lst

    bank, ref = w.new_bank(3, config=config), w.new_bank(3, config=config)
    r0, r1, lst = prepare(bank)
    prepare(ref)
    r0 = lst[1]   # member 0's result is now the list's last entry that named it
    assert np.array_equal(bank.result(0, 1)[0], r0)
    prev = bank.select([w.selector(bank, 1, 1)], [host_srcs(pkg, 2, first=2)], host_words=cts)[0]
    assert np.array_equal(prev, w.oselect(1, cts[2:4], w.index_digits(1, 1)))
    srcs = [S.member(0), S.member(1), S.list(0), S.list(2), S.select(0), S.zero(), S.host(0), S.host(1)]
    cand = np.stack([r0, r1, lst[0], lst[2], prev, np.zeros_like(prev), cts[0], cts[1]])
    sels = [w.selector(bank, idx, 3) for idx in range(8)]
    got = bank.select(sels, [srcs] * 8, host_words=cts)
    for idx in range(8):
        want = w.oselect(3, cand, w.index_digits(idx, 3))
        assert np.array_equal(got[idx], want), (idx, np.count_nonzero(got[idx] != want))
    # nothing of the bank moved: results, the list's results, state flags; and member 1 resumes its write
    assert np.array_equal(bank.result(0, 3), np.stack([r0, r1, lst[2]]))
    assert np.array_equal(bank.list_result(0, 3), lst)
    assert [bank.state(m) for m in range(3)] == [False, True, False]
    for bk in (bank, ref):
        bk.write(cts[3:4], [a[1]], w.keys, first=1)
    for m in range(3):
        assert np.array_equal(bank.store_encrypted(m), ref.store_encrypted(m)), m
    assert np.array_equal(bank.read([a[1]], w.keys, first=1), ref.read([a[1]], w.keys, first=1))


# ---- 4. several selects in one call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 4])
def test_several_selects_equal_the_single_selects(w2, bank2, n):
    """select k of the call has shape SHAPE (b = 5, m = 20, two digits: the table form of the tail launch) with its own index and a rotated candidate list"""
    w, pkg = w2, w2.pkg
    b, m = 5, 20
    vals, cts = w.candidates(m)
    idxs = [0, 19, 10, 20][:n]
    sels = [w.selector(bank2, idx, b) for idx in idxs]
    got = bank2.select(sels, [host_srcs(pkg, m)] * n, host_words=cts)
    assert got.shape == (n, w.ws, w.params.glwe_len())
    for k, idx in enumerate(idxs):
        assert np.array_equal(got[k], single(w, bank2, b, m, idx)[0]), (n, k)
    # candidate lists of different lengths in one call (b = 3: m = 8, 3, 1, 5)
    ms = [8, 3, 1, 5][:n]
    idx3 = [7, 2, 0, 6][:n]
    off = np.cumsum([0] + ms)
    srcs = [[pkg.Src.host(int(off[k]) + j) for j in range(ms[k])] for k in range(n)]
    got = bank2.select([w.selector(bank2, i, 3) for i in idx3], srcs, host_words=cts)
    for k in range(n):
        want = w.oselect(3, cts[off[k]:off[k + 1]], w.index_digits(idx3[k], 3))
        assert np.array_equal(got[k], want), (n, k)


def test_mixed_bits_are_refused_and_64_ciphertexts_are_accepted(po, w2, bank2):
    w, pkg = w2, w2.pkg
    vals, cts = w.candidates(2)
    with pytest.raises(pkg.FheRamError) as e:
        bank2.select([w.selector(bank2, 0, 1), w.selector(bank2, 0, 2)], [host_srcs(pkg, 2)] * 2, host_words=cts)
    assert e.value.code == ST_INVALID_ARG and "bits" in e.value.msg
    # n * ws = 64: word size 8, eight selects of two candidates
    w8 = SelWorld(po, 1 << 12, 1, 8, seed=330)
    bank = w8.new_bank(1)
    bank._use_keys(w8.keys)
    vals8, cts8 = w8.candidates(2)
    idxs = [0, 1, 1, 0, 1, 0, 0, 1]
    got = bank.select([w8.selector(bank, i, 1) for i in idxs], [host_srcs(pkg, 2)] * 8, host_words=cts8)
    want = {i: w8.oselect(1, cts8, w8.index_digits(i, 1)) for i in (0, 1)}
    for k, i in enumerate(idxs):
        assert np.array_equal(got[k], want[i]), k
    w8.check_value(got[7], vals8[1])
    with pytest.raises(pkg.FheRamError) as e:   # nine selects
        bank.select([w8.selector(bank, 0, 1)] * 9, [host_srcs(pkg, 2)] * 9, host_words=cts8)
    assert e.value.code == ST_INVALID_ARG


# ---- 5. forced forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [{"safe": 1}, {"tail": 0}, {"fuse": 0}, {"graph": 1}, {"monitor": 2}, {"tail_ep": 0}, {"limb_split": 0}],
                         ids=["safe", "tail0", "fuse0", "graph", "monitor2", "tail_ep0", "limb_split0"])
def test_forced_forms_give_the_same_integers(w2, bank2, config):
    w, pkg = w2, w2.pkg
    b, m = 5, 20
    vals, cts = w.candidates(m)
    bank = w.new_bank(3, config=config)
    bank._use_keys(w.keys)
    for idx, n in ((10, 1), (19, 3)):   # one select (no table) and three (the table forms)
        got = bank.select([w.selector(bank, idx, b)] * n, [host_srcs(pkg, m)] * n, host_words=cts)
        want = single(w, bank2, b, m, idx)
        assert np.array_equal(want[0], want[1])
        for k in range(n):
            assert np.array_equal(got[k], want[1]), (config, idx, k, np.count_nonzero(got[k] != want[1]))
    assert bank.roundoff_max() < 0.375


# ---- 6. extreme limbs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["min", "max", "alternating"])
def test_extreme_limbs_pack_as_the_oracle_normalises(w1, pattern):
    """32 candidates whose every limb is -2^16, 2^16 - 1, or both in turn: the un-normalised sum reaches 32 * 2^16 = 2^21 per limb (int32 holds it);
    the output equals the oracle's read of the oracle's glwe_normalize of the same sum, under monitor = 2 (every coefficient watched)"""
    w, pkg = w1, w1.pkg
    glen = w.params.glwe_len()
    lo, hi = -(1 << 16), (1 << 16) - 1
    if pattern == "min":
        cts = np.full((32, 1, glen), lo, dtype=np.int64)
    elif pattern == "max":
        cts = np.full((32, 1, glen), hi, dtype=np.int64)
    else:
        cts = np.where((np.arange(32)[:, None, None] + np.arange(glen)[None, None, :]) % 2 == 0, lo, hi).astype(np.int64)
    bank = w.new_bank(1, config={"monitor": 2})
    bank._use_keys(w.keys)
    ob = w.small(5)[0]
    packed = ob.glwe_normalize(sum(ob.glwe_rotate(j, cts[j][0]) for j in range(32)))
    assert np.abs(sum(ob.glwe_rotate(j, cts[j][0]) for j in range(32))).max() > (1 << 17)   # the normalisation is not optional
    for idx in (0, 21):
        got = bank.select([w.selector(bank, idx, 5)], [host_srcs(pkg, 32)], host_words=cts)
        want = w.oselect(5, cts, w.index_digits(idx, 5))
        assert np.array_equal(got[0], want), (pattern, idx, np.count_nonzero(got[0] != want))
    ro = bank.roundoff_max()
    print(f"extreme limbs ({pattern}): round-off maximum {ro:.4f}")
    assert ro < 0.375


# ---- 7. the conditional write: a VM step's write enable ----------------------------------------------------------------------------------
_COND = {}
ENABLE = 0b01   # member 0 (bit 0): write the new word; member 2 (bit 1): keep the old one
MEMBERS = [0, 2]


def cond_oracle(w):
    """the oracle Rams of members 0 and 2 driven with the oracle's select output as w: rows, tree, state, read-back, the select outputs"""
    if id(w) not in _COND:
        vals, new = w.candidates(2, seed=42)
        out = {"new_vals": vals}
        for k, m in enumerate(MEMBERS):
            oram, oa = w.new_oram(m), w.o.address_new(w.addr_g[k])
            old = oram.read_prepare_write(oa, w.okeys)
            pick = w.oselect(1, np.stack([old, new[k]]), w.digits(ENABLE, k, 1))
            oram.write(pick, oa, w.okeys)
            out[m] = {"old": old, "pick": pick, "rows": oram.store(), "tree": oram.tree(0), "state": oram.state, "readback": oram.read(oa, w.okeys)}
        _COND[id(w)] = out
    return _COND[id(w)]


@pytest.mark.parametrize("variant", ["device_words", "read_list_between", "host_words"])
def test_conditional_write(w13, variant):
    w, pkg, S = w13, w13.pkg, w13.pkg.Src
    want = cond_oracle(w)
    vals, new = w.candidates(2, seed=42)
    bank = w.new_bank(3)
    before1 = (sha(bank.store_encrypted(1)), sha(bank.tree(1, 0)), bank.state(1))
    addrs = [w.addrs[0], w.addrs[1]]
    fu = pkg.FheUintPrepared.from_host(bank, w.bits(ENABLE))
    sels = [bank.selector(1), bank.selector(1)]
    assert bank.read_prepare_write_list(MEMBERS, addrs, w.keys, download=False) is None
    bank.derive_selectors([fu, fu], [0, 1], sels)
    if variant == "read_list_between":
        between = bank.read_list([1], [w.addrs[2]], w.keys)
    picks = bank.select(sels, [[S.member(0), S.host(0)], [S.member(2), S.host(1)]], host_words=new, download=(variant == "host_words"))
    if variant == "host_words":
        bank.write_list(MEMBERS, picks, addrs, w.keys)
    else:
        bank.write_list_selected(MEMBERS, [0, 1], addrs, w.keys)
        picks = bank.select_result(0, 2)
    for k, m in enumerate(MEMBERS):
        assert np.array_equal(picks[k], want[m]["pick"]), (variant, "select output", m)
        assert np.array_equal(bank.result(m, 1)[0], want[m]["old"]), (variant, "old", m)
        assert bank.state(m) == want[m]["state"] is False
        assert np.array_equal(np.ravel(bank.store_encrypted(m)), np.ravel(want[m]["rows"])), (variant, "rows", m)
        assert np.array_equal(bank.tree(m, 0), want[m]["tree"]), (variant, "tree", m)
    got = bank.read_list(MEMBERS, addrs, w.keys)
    for k, m in enumerate(MEMBERS):
        assert np.array_equal(got[k], want[m]["readback"]), (variant, "read-back", m)
    # the write enable did what it says: member 0 holds the new word, member 2 its old one
    w.check_value(got[0], vals[0], "enabled")
    w.check_word(got[1], w.data[2], 1)
    assert (sha(bank.store_encrypted(1)), sha(bank.tree(1, 0)), bank.state(1)) == before1, "member 1 was touched"
    if variant == "read_list_between":
        assert np.array_equal(between[0], w.new_oram(1).read(w.o.address_new(w.addr_g[2]), w.okeys))


def test_move_between_members(w13):
    """lw / sw: a read-list entry of member 2 -> select with one candidate (b = 1, index 0) -> write_list_selected into member 0"""
    w, pkg, S = w13, w13.pkg, w13.pkg.Src
    bank = w.new_bank(3)
    bank.read_prepare_write([w.addrs[0]], w.keys, first=0, download=False)
    src = bank.read_list([1, 2], [w.addrs[2], w.addrs[1]], w.keys)[1]
    out = bank.select([w.selector(bank, 0, 1)], [[S.list(1)]])
    assert np.array_equal(out[0], w.oselect(1, src[None], w.index_digits(0, 1)))
    bank.write_list_selected([0], [0], [w.addrs[0]], w.keys)
    back = bank.read([w.addrs[0]], w.keys, first=0)[0]
    w.check_word(back, w.data[2], 1, written=False)   # what member 2 holds at address 1, now in member 0 at address 0
    for i in range(w.ws):
        assert w.o.glwe_decrypt(back[i], 0, w.sk)[0] == w.o.glwe_decrypt(src[i], 0, w.sk)[0]


def test_one_member_bank_enqueues_a_whole_step_without_a_sync(w13):
    """a bank of one member is a plain context (pre_inv in effect): read_prepare_write, derive, select, write_list_selected back to back with no
    host wait equal the same sequence with a wait after each"""
    w, pkg, S = w13, w13.pkg, w13.pkg.Src
    vals, new = w.candidates(1, seed=43)
    outs = []
    for sync in (False, True):
        bank = w.new_bank(1)
        fu = pkg.FheUintPrepared.from_host(bank, w.bits(ENABLE))
        sel = bank.selector(1)
        bank.sync()
        for step in (lambda: bank.read_prepare_write([w.addrs[0]], w.keys, download=False),
                     lambda: bank.derive_selectors([fu], [0], [sel]),
                     lambda: bank.select([sel], [[S.member(0), S.host(0)]], host_words=new, download=False),
                     lambda: bank.write_list_selected([0], [0], [w.addrs[0]], w.keys)):
            step()
            if sync:
                bank.sync()
        bank.sync()
        outs.append((bank.select_result(0, 1), bank.store_encrypted(0), bank.tree(0, 0), bank.state(0), bank.read([w.addrs[0]], w.keys)))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    w.check_value(outs[0][4][0], vals[0], "written")
    want = cond_oracle(w)[0]   # member 0 with enable bit 1 and the same old word; the new word differs, so only the old side is shared
    assert np.array_equal(w.new_bank(1).read_prepare_write([w.addrs[0]], w.keys)[0], want["old"])


# ---- 8. launch profile ------------------------------------------------------------------------------------------------------------------------
def test_launch_profile(w2, bank2):
    w, pkg = w2, w2.pkg
    vals, cts = w.candidates(20)
    for n, b, m in ((1, 5, 20), (4, 5, 20), (3, 1, 2)):
        sels = [w.selector(bank2, k, b) for k in range(n)]
        bank2.sync()
        bank2.profile_reset()
        bank2.profile_enable(True)
        bank2.select(sels, [host_srcs(pkg, m)] * n, host_words=cts)
        prof = bank2.profile_get("select_pack")
        bank2.profile_enable(False)
        assert prof["launches"] == 1 and prof["blocks"] == n * w.ws, (n, b, m, prof)


# ---- 9. refusals: all host-side, before anything is enqueued ------------------------------------------------------------------------------
def test_refusals_change_nothing(w2, w1):
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    L = lib()
    vals, cts = w.candidates(4)
    bank = w.new_bank(3)
    other = w1.new_bank(1)
    fresh = w.new_bank(3)   # keys not loaded, nothing run
    bank.read([w.addrs[0]], w.keys, first=0)
    lst = bank.read_list([1, 0], [w.addrs[1], w.addrs[2]], w.keys)
    sel = w.selector(bank, 1, 2)
    foreign = w1.selector(other, 1, 2)
    empty = bank.selector(2)
    fu = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))
    fu10 = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE)[:10])
    fu_other = pkg.FheUintPrepared.from_host(other, w1.bits(VALUE))

    def digest():
        return ([sha(bank.store_encrypted(m)) for m in range(3)], [bank.state(m) for m in range(3)], sha(bank.result(0, 3)), sha(bank.list_result(0, 2)),
                sha(sel.download()))

    before = digest()

    def refused(code, call, what):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg, what

    ok = [S.host(0), S.host(1), S.host(2)]
    # -- selectors
    refused(ST_INVALID_ARG, lambda: bank.selector(0), "bits 0")
    refused(ST_INVALID_ARG, lambda: bank.selector(6), "bits 6")
    refused(ST_INVALID_ARG, lambda: pkg.Selector.from_digits(bank, 5, list(w.index_digits(1, 2))), "n_ggsw != the plan's digit count")
    refused(ST_INVALID_ARG, lambda: pkg.Selector.from_digits(bank, 2, []), "no digits")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu_other], [0], [sel]), "integer of another bank")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu], [0], [foreign]), "selector of another bank")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu], [31], [sel]), "first_bit + bits beyond the width")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu10], [9], [sel]), "first_bit + bits beyond a narrow integer")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu], [-1], [sel]), "negative first_bit")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu, fu], [0, 4], [sel, sel]), "the same selector twice")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu] * 9, [0] * 9, [bank.selector(2) for _ in range(9)]), "n = 9")
    refused(ST_INVALID_ARG, lambda: foreign.bank.select([sel], [ok], host_words=cts), "select with a selector of another bank")
    assert L.fheram_bank_selector_alloc(bank._h, 2, None) == ST_INVALID_ARG
    assert L.fheram_bank_selector_derive(bank._h, None, None, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_selector_download(bank._h, sel._h, None) == ST_INVALID_ARG
    refused(ST_INVALID_ARG, empty.download, "download of an underived selector")
    # -- select
    refused(ST_INVALID_ARG, lambda: bank.select([empty], [ok], host_words=cts), "underived selector")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.host(j) for j in range(4)] + [S.zero()]], host_words=cts), "n_cand > 2^bits")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S(9, 0)]], host_words=cts), "unknown source kind")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.member(3)]]), "member outside the bank")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.member(-1)]]), "negative member")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.list(2)]]), "entry outside the last list")
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.host(0)]]), "HOST without host_words")
    refused(ST_INVALID_ARG, lambda: bank.select([sel] * 9, [ok] * 9, host_words=cts), "n = 9")
    n_cand, p1 = (C.c_int * 1)(0), (C.c_void_p * 1)(sel._h)
    src1 = (pkg.api._CSelectSrc * 1)(pkg.api._CSelectSrc(0, 0))
    assert L.fheram_bank_select(bank._h, p1, n_cand, 1, src1, None, None) == ST_INVALID_ARG   # n_cand = 0
    assert L.fheram_bank_select(bank._h, None, n_cand, 1, src1, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_select(bank._h, p1, None, 1, src1, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_select(bank._h, p1, n_cand, 1, None, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_select(bank._h, p1, n_cand, 0, src1, None, None) == ST_INVALID_ARG
    refused(ST_STATE, lambda: bank.select([sel], [[S.member(2)]]), "a member without a result")
    refused(ST_STATE, lambda: bank.select([sel], [[S.select(0)]]), "no select has run")
    refused(ST_STATE, lambda: bank.select_result(0, 1), "select_result before any select")
    bad = cts.copy()
    bad[1, 0, 5] = (1 << 16) + 1
    refused(ST_RANGE, lambda: bank.select([sel], [ok], host_words=bad), "host limb out of range")
    bank.select([sel], [[S.host(0)]], host_words=bad, download=False)   # ... in a slot no source names: not looked at
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.select(1)]]), "output outside the last select")
    refused(ST_INVALID_ARG, lambda: bank.select_result(1, 1), "select_result outside the last select")
    assert L.fheram_bank_select_result(bank._h, 0, 1, None) == ST_INVALID_ARG
    fsel = w.selector(fresh, 1, 2)
    refused(ST_KEYS, lambda: fresh.select([fsel], [ok], host_words=cts), "keys not loaded")
    refused(ST_STATE, lambda: fresh.select([fsel], [[S.list(0)]], keys=w.keys), "no read list has run")
    # -- write_list_selected: the checks of write_list, and its own
    refused(ST_STATE, lambda: bank.write_list_selected([0], [0], [w.addrs[0]], w.keys), "member in state 0")
    refused(ST_INVALID_ARG, lambda: bank.write_list_selected([0, 0], [0, 0], [w.addrs[0]] * 2, w.keys), "a member named twice")
    assert L.fheram_bank_write_list_selected(bank._h, None, None, 1, None) == ST_INVALID_ARG
    assert digest() == before
    bank.read_prepare_write([w.addrs[0]], w.keys, first=0, download=False)
    prepared = [sha(bank.store_encrypted(m)) for m in range(3)]   # (read_prepare_write rotates the rows of a one-row RAM in place, ram.rs:502-504)
    refused(ST_INVALID_ARG, lambda: bank.write_list_selected([0], [1], [w.addrs[0]], w.keys), "a pick outside the last select")
    refused(ST_INVALID_ARG, lambda: bank.write_list_selected([0], [-1], [w.addrs[0]], w.keys), "a negative pick")
    fresh.read_prepare_write([w.addrs[0]], w.keys, first=0, download=False)
    refused(ST_STATE, lambda: fresh.write_list_selected([0], [0], [w.addrs[0]], w.keys), "no select has run")
    assert bank.state(0) is True and [sha(bank.store_encrypted(m)) for m in range(3)] == prepared
    bank.write_list_selected([0], [0], [w.addrs[0]], w.keys)   # ... and the prepared member still takes its write
    assert bank.state(0) is False


def test_allocation_failure_is_reported_and_the_next_call_works(w2):
    """the select's buffers follow the lists' pattern (allocated on first use, grown to the largest call): a failing allocation is
    FHERAM_ERR_DEVICE, nothing is kept of the failed growth, and every later call works"""
    w, pkg = w2, w2.pkg
    vals, cts = w.candidates(2)
    bank = w.new_bank(3)
    bank._use_keys(w.keys)
    sel = w.selector(bank, 1, 1)
    args = dict(host_words=cts)
    for nth in (1, 6):
        bank.selftest_fail_select_alloc(nth)
        with pytest.raises(pkg.FheRamError) as e:
            bank.select([sel], [host_srcs(pkg, 2)], **args)
        assert e.value.code == ST_DEVICE, e.value
    want = w.oselect(1, cts, w.index_digits(1, 1))
    assert np.array_equal(bank.select([sel], [host_srcs(pkg, 2)], **args)[0], want)
    bank.selftest_fail_select_alloc(2)   # growth to three selects fails: the last select's output is still there, and a call that fits still works
    with pytest.raises(pkg.FheRamError) as e:
        bank.select([sel] * 3, [host_srcs(pkg, 2)] * 3, **args)
    assert e.value.code == ST_DEVICE
    assert np.array_equal(bank.select_result(0, 1)[0], want)
    assert np.array_equal(bank.select([sel], [[pkg.Src.select(0), pkg.Src.host(0)]], **args)[0],
                          w.oselect(1, np.stack([want, cts[0]]), w.index_digits(1, 1)))
    got = bank.select([sel] * 3, [host_srcs(pkg, 2)] * 3, **args)   # the growth itself, with the previous output moved over
    assert all(np.array_equal(got[k], want) for k in range(3))
    assert np.array_equal(bank.read([w.addrs[0]], w.keys, first=0)[0], w.new_oram(0).read(w.o.address_new(w.addr_g[0]), w.okeys))
