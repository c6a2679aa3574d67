"""Sub-word loads and stores on the device (include/fheram.h): fheram_bank_select_lanes (RamBank.select_lanes), field selectors
(RamBank.selector_fields, Selector.from_digits_fields, RamBank.derive_selector_fields) and addresses from a bit offset
(derive_addresses(first_bits=...)).

The contract, in operations the parent already has and in the oracle's own:
  (a) identity lanes (lane = w, one source per candidate) give what fheram_bank_select gives on the same sources;
  (b) any lanes give what fheram_bank_select gives on HOST candidates the host assembled from the downloaded source words with the lanes
      permuted, and what the oracle recipe of test_gpu_select.py (SelWorld.oselect) gives on those assembled words;
  a field selector of widths W is the Address of an oracle whose decomp_n is W padded to log N, from the concatenated bit fields.
Every comparison is np.array_equal on int64; the noise of decrypted outputs is printed, not bounded (DESIGN.md 15 records it).
Banks are at max_addr = 2^12 (one row, one coordinate) unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import lib, sha
from test_gpu_select import ST_DEVICE, ST_INVALID_ARG, ST_KEYS, ST_RANGE, ST_STATE, VALUE, SelWorld, host_srcs
from test_lanes_abi import c_want

pytestmark = pytest.mark.gpu

VALUE_B = 0x4A1C5926   # a second encrypted integer: field selectors take their fields from two
PADDED = {(2, 2): (16, [2, 2, 2, 2, 2, 2]), (1, 3): (16, [1, 3, 2, 3, 3]), (2, 3): (32, [2, 3, 1, 3, 3]), (1, 1, 1): (8, [1, 1, 1, 3, 3, 3])}   # widths -> (2^bits, decomp_n)


class LaneWorld(SelWorld):
    """a SelWorld plus the oracles of field selectors and the host-side assembly of lane-mapped candidates"""

    def __init__(self, po, max_addr, n_members, word_size, seed, **crypto):
        super().__init__(po, max_addr, n_members, word_size, seed, **crypto)
        self._field, self._fdigits = {}, {}

    def field_oracle(self, widths):
        """(oracle of max_addr = 2^sum(widths) whose decomp_n starts with widths, its prepared keys)"""
        key = tuple(widths)
        if key not in self._field:
            max_addr, padded = PADDED[key]
            assert max_addr == 1 << sum(widths) and sum(padded) == 12
            assert self.po.get_base_2d(max_addr, padded) == [list(widths)]   # a plan the oracle reads differently fails here, loudly
            ob = self.po.Oracle(self.oparams(max_addr, decomp_n=padded))
            assert ob.n_digits == len(widths)
            self._field[key] = (ob, ob.keys_prepare(self.evk))
        return self._field[key]

    def field_digits(self, widths, values, firsts):
        """digit d from bits [firsts[d], firsts[d] + widths[d]) of values[d]: [n_fields][ggsw_len]"""
        key = (tuple(widths), tuple(values), tuple(firsts))
        if key not in self._fdigits:
            bits = np.concatenate([self.bits(v)[f:f + wd] for v, f, wd in zip(values, firsts, widths)])
            self._fdigits[key] = self.field_oracle(widths)[0].address_from_fheuint(bits, sign=False)
        return self._fdigits[key]

    def oselect_fields(self, widths, cands, digits):
        """SelWorld.oselect with the field oracle: cands [m][ws][GLWE] int64 -> [ws][GLWE]"""
        ob, okeys = self.field_oracle(widths)
        cands = np.asarray(cands, dtype=np.int64)
        packed = np.stack([ob.glwe_normalize(sum(ob.glwe_rotate(j, cands[j][y]) for j in range(cands.shape[0]))) for y in range(self.ws)])
        oram = ob.ram_new()
        oram.load(packed.reshape(self.ws, 1, -1))
        return oram.read(ob.address_new(digits), okeys)

    def assemble(self, cands, sources):
        """the words the host puts together: cands [m][ws] Lane, sources {(kind, index): [ws][GLWE]} -> [m][ws][GLWE]"""
        zero = np.zeros(self.params.glwe_len(), dtype=np.int64)
        return np.stack([np.stack([zero if l.kind == 0 else sources[(l.kind, l.index)][l.lane] for l in c]) for c in cands])


def identity(pkg, srcs, ws):
    return [[pkg.Lane.of(s, w) for w in range(ws)] for s in srcs]


def host_sources(cts):
    return {(1, i): cts[i] for i in range(len(cts))}


@pytest.fixture(scope="module")
def w2(po):
    return LaneWorld(po, 1 << 12, 3, 2, seed=400)


@pytest.fixture(scope="module")
def w4(po):
    return LaneWorld(po, 1 << 12, 3, 4, seed=410)


@pytest.fixture(scope="module")
def w13(po):
    return LaneWorld(po, 1 << 13, 3, 4, seed=420)


@pytest.fixture(scope="module")
def bank4(w4):
    """one default bank of three members (word size 4) shared by the tests that change no member"""
    bank = w4.new_bank(3)
    bank._use_keys(w4.keys)
    return bank


# ---- 1. identity (a): identity lanes are fheram_bank_select -------------------------------------------------------------------------------
def test_identity_lanes_equal_select_for_every_source_kind(w2):
    """ws = 2, m = 3 / b = 2, two selects in one call over: a member's read result, a member's read_prepare_write result, a read-list entry,
    the previous select's output, ZERO and a host word"""
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    vals, cts = w.candidates(4, seed=41)
    a = w.addrs
    bank = w.new_bank(3)
    bank.read([a[0]], w.keys, first=0)
    bank.read_prepare_write([a[1]], w.keys, first=1)
    lst = bank.read_list([2, 2], [a[2], a[0]], w.keys)
    srcs = [[S.member(0), S.list(1), S.select(0)], [S.zero(), S.host(1), S.member(1)]]
    sels = [w.selector(bank, 2, 2), w.selector(bank, 1, 2)]

    def previous():
        return bank.select([w.selector(bank, 1, 1)], [host_srcs(pkg, 2, first=2)], host_words=cts)[0]

    prev = previous()
    want = bank.select(sels, srcs, host_words=cts)
    assert np.array_equal(previous(), prev)
    got = bank.select_lanes(sels, [identity(pkg, s, w.ws) for s in srcs], host_words=cts)
    assert got.shape == (2, w.ws, w.params.glwe_len())
    assert np.array_equal(got, want), np.count_nonzero(got != want)
    assert np.array_equal(got[0], w.oselect(2, np.stack([bank.result(0, 1)[0], lst[1], prev]), w.index_digits(2, 2)))
    assert np.array_equal(bank.select_result(0, 2), want), "a lanes select is the last select"
    # nothing of the bank moved, and the prepared member still takes its write
    assert np.array_equal(bank.list_result(0, 2), lst)
    assert [bank.state(m) for m in range(3)] == [False, True, False]
    bank.write_list_selected([1], [1], [a[1]], w.keys)
    ref = w.new_bank(3)
    ref.read_prepare_write([a[1]], w.keys, first=1)
    ref.write(want[1:2], [a[1]], w.keys, first=1)
    assert np.array_equal(bank.store_encrypted(1), ref.store_encrypted(1))


# ---- 2. identity (b): any lanes are select on the host-assembled words, and the oracle's recipe on them -----------------------------------
def lane_cases(pkg):
    L = pkg.Lane
    h = lambda i, perm: [L.host(i, p) for p in perm]   # noqa: E731
    return {
        "permute": [h(0, [1, 0, 3, 2]), h(1, [1, 0, 3, 2]), h(2, [3, 2, 1, 0])],
        "repeat": [h(0, [2, 2, 2, 2]), h(1, [0, 0, 0, 0]), h(2, [3, 3, 3, 3])],
        "mix": [[L.host(0, 0), L.member(0, 0), L.host(0, 2), L.host(0, 3)], [L.list_entry(1, 3), L.list_entry(1, 2), L.host(1, 1), L.member(0, 1)],
                [L.member(0, 2), L.member(0, 3), L.list_entry(0, 0), L.list_entry(0, 1)]],
        "zero": [[L.zero(), L.host(0, 0), L.zero(), L.host(0, 1)], [L.zero()] * 4, [L.host(2, 3), L.zero(), L.zero(), L.zero()]],
    }


@pytest.fixture(scope="module")
def mixbank(w4):
    """a bank with a member result and a read list, and their downloads"""
    w = w4
    bank = w.new_bank(3)
    res0 = bank.read([w.addrs[0]], w.keys, first=0)[0]
    lst = bank.read_list([1, 2], [w.addrs[1], w.addrs[2]], w.keys)
    vals = {(2, 0): [w.data[0][i + 4 * w.idx[0]] for i in range(4)], (3, 0): [w.data[1][i + 4 * w.idx[1]] for i in range(4)],
            (3, 1): [w.data[2][i + 4 * w.idx[2]] for i in range(4)]}
    return bank, {(2, 0): res0, (3, 0): lst[0], (3, 1): lst[1]}, vals


@pytest.mark.parametrize("case", ["permute", "repeat", "mix", "zero"])
def test_lanes_equal_select_on_assembled_host_words_and_the_oracle(w4, mixbank, case):
    w, pkg = w4, w4.pkg
    bank, sources, svals = mixbank
    vals, cts = w.candidates(3)
    sources = {**sources, **host_sources(cts)}
    svals = {**svals, **{(1, i): vals[i] for i in range(3)}}
    cands = lane_cases(pkg)[case]
    words = w.assemble(cands, sources)
    b, m = 2, 3
    for idx in (0, m - 1, m):   # an index >= m selects zero
        sel = w.selector(bank, idx, b)
        got = bank.select_lanes([sel], [cands], host_words=cts)[0]
        want = bank.select([sel], [host_srcs(pkg, m)], host_words=words)[0]
        assert np.array_equal(got, want), (case, idx, np.count_nonzero(got != want))
        assert np.array_equal(got, w.oselect(b, words, w.index_digits(idx, b))), (case, idx)
        values = None if idx >= m else [0 if l.kind == 0 else svals[(l.kind, l.index)][l.lane] for l in cands[idx]]
        noise = w.check_value(got, values, (case, idx))
        print(f"lanes {case} idx={idx}: log2 noise {noise:.2f}")
    assert np.array_equal(bank.result(0, 1)[0], sources[(2, 0)]) and np.array_equal(bank.list_result(0, 2), np.stack([sources[(3, 0)], sources[(3, 1)]]))


# ---- 3. table-size edges --------------------------------------------------------------------------------------------------------------------
def test_one_candidate_and_thirty_two(w4, bank4):
    """m = 1; m = 32 / b = 5 at ws = 4: 128 pointers, more than the by-value argument struct of k_select_pack held per select"""
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    vals, cts = w.candidates(32, seed=50)
    one = [[L.host(5, 3), L.host(4, 0), L.zero(), L.host(5, 1)]]
    words = w.assemble(one, host_sources(cts))
    got = bank4.select_lanes([w.selector(bank4, 0, 1)], [one], host_words=cts)[0]
    assert np.array_equal(got, w.oselect(1, words, w.index_digits(0, 1)))
    w.check_value(got, [vals[5][3], vals[4][0], 0, vals[5][1]], "m = 1")
    cands = [[L.host((j + 3 * wd) % 32, (wd + j) % 4) for wd in range(4)] for j in range(32)]
    words = w.assemble(cands, host_sources(cts))
    for idx in (0, 31):
        sel = w.selector(bank4, idx, 5)
        got = bank4.select_lanes([sel], [cands], host_words=cts)[0]
        assert np.array_equal(got, bank4.select([sel], [host_srcs(pkg, 32)], host_words=words)[0]), idx
        assert np.array_equal(got, w.oselect(5, words, w.index_digits(idx, 5))), idx
        w.check_value(got, [vals[l.index][l.lane] for l in cands[idx]], ("m = 32", idx))


def test_eight_selects_with_different_candidate_counts(w4, bank4):
    """n = 8 at ws = 4 (n * ws = 32) with n_cand = 8, 3, 1, 5, 2, 7, 4, 6: the offsets into the lane list"""
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    vals, cts = w.candidates(32, seed=50)
    ms, idxs = [8, 3, 1, 5, 2, 7, 4, 6], [7, 2, 0, 5, 1, 0, 3, 6]   # (index 5 of 5 candidates: zero)
    off = np.cumsum([0] + ms)
    cands = [[[L.host((int(off[k]) + j) % 32 if wd % 2 else 31 - j, (wd + k) % 4) for wd in range(4)] for j in range(ms[k])] for k in range(8)]
    sels = [w.selector(bank4, i, 3) for i in idxs]
    got = bank4.select_lanes(sels, cands, host_words=cts)
    flat = [c for cs in cands for c in cs]
    words = w.assemble(flat, host_sources(cts))
    want = bank4.select(sels, [host_srcs(pkg, ms[k], first=int(off[k])) for k in range(8)], host_words=words)
    assert np.array_equal(got, want), [int(np.count_nonzero(got[k] != want[k])) for k in range(8)]
    for k in (0, 3, 7):
        assert np.array_equal(got[k], w.oselect(3, words[off[k]:off[k + 1]], w.index_digits(idxs[k], 3))), k


def test_sixty_four_output_ciphertexts(po):
    """n * ws = 64: word size 8, eight selects; the ninth is refused"""
    w = LaneWorld(po, 1 << 12, 1, 8, seed=430)
    pkg, L = w.pkg, w.pkg.Lane
    bank = w.new_bank(1)
    bank._use_keys(w.keys)
    vals, cts = w.candidates(2)
    cands = [[L.host(0, 7 - wd) for wd in range(8)], [L.host(1, (wd + 3) % 8) for wd in range(8)]]
    words = w.assemble(cands, host_sources(cts))
    idxs = [0, 1, 1, 0, 1, 0, 0, 1]
    got = bank.select_lanes([w.selector(bank, i, 1) for i in idxs], [cands] * 8, host_words=cts)
    want = {i: w.oselect(1, words, w.index_digits(i, 1)) for i in (0, 1)}
    for k, i in enumerate(idxs):
        assert np.array_equal(got[k], want[i]), k
    w.check_value(got[7], [vals[1][(wd + 3) % 8] for wd in range(8)])
    with pytest.raises(pkg.FheRamError) as e:
        bank.select_lanes([w.selector(bank, 0, 1)] * 9, [cands] * 9, host_words=cts)
    assert e.value.code == ST_INVALID_ARG


# ---- 4. full-polynomial candidates: the negacyclic wrap of X^j and the carry pass on every coefficient ------------------------------------
@pytest.mark.parametrize("pattern", ["random", "alternating"])
def test_full_polynomial_candidates(w2, pattern):
    """32 candidates whose every coefficient is a normalised limb (random, or -2^16 / 2^16 - 1 in turn: the un-normalised sum reaches 2^21), with
    the two lanes of every word swapped, under monitor = 2"""
    w, pkg, L = w2, w2.pkg, w2.pkg.Lane
    glen = w.params.glwe_len()
    lo, hi = -(1 << 16), (1 << 16) - 1
    if pattern == "random":
        cts = np.random.default_rng(77).integers(lo, hi + 1, size=(32, 2, glen), dtype=np.int64)
    else:
        cts = np.where((np.arange(32)[:, None, None] + np.arange(2)[None, :, None] + np.arange(glen)[None, None, :]) % 2 == 0, lo, hi).astype(np.int64)
    bank = w.new_bank(1, config={"monitor": 2})
    bank._use_keys(w.keys)
    cands = [[L.host(j, 1), L.host(31 - j, 0)] for j in range(32)]
    words = w.assemble(cands, host_sources(cts))
    ob = w.small(5)[0]
    assert np.abs(sum(ob.glwe_rotate(j, words[j][0]) for j in range(32))).max() > (1 << 17)   # the normalisation is not optional
    for idx in (0, 21):
        sel = w.selector(bank, idx, 5)
        got = bank.select_lanes([sel], [cands], host_words=cts)[0]
        assert np.array_equal(got, bank.select([sel], [host_srcs(pkg, 32)], host_words=words)[0]), (pattern, idx)
        assert np.array_equal(got, w.oselect(5, words, w.index_digits(idx, 5))), (pattern, idx)
    ro = bank.roundoff_max()
    print(f"full-polynomial candidates ({pattern}): round-off maximum {ro:.4f}")
    assert ro < 0.375


# ---- 5. no host wait -----------------------------------------------------------------------------------------------------------------------
def test_two_lanes_calls_back_to_back_then_the_write(w4):
    """two lanes calls with out == NULL (the second overwrites the pinned pointer table behind its event), select_result, and
    write_list_selected from the second: rows equal a bank that downloads, assembles on the host and writes with write_list"""
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    vals, cts = w.candidates(3)
    bank, ref = w.new_bank(3), w.new_bank(3)
    a = w.addrs
    for bk in (bank, ref):
        bk.read_prepare_write([a[0]], w.keys, first=0, download=False)
    old = ref.result(0, 1)[0]
    first = [[L.host(0, 3), L.host(0, 2), L.host(0, 1), L.host(0, 0)], [L.host(1, wd) for wd in range(4)]]
    second = [[L.member(0, 0), L.host(2, 0), L.member(0, 2), L.member(0, 3)], [L.host(2, wd) for wd in range(4)], [L.member(0, wd) for wd in range(4)]]
    s1, s2 = w.selector(bank, 1, 1), w.selector(bank, 0, 2)
    assert bank.select_lanes([s1], [first], host_words=cts, download=False) is None
    assert bank.select_lanes([s2, s2], [second, second[1:]], host_words=cts, download=False) is None
    bank.write_list_selected([0], [0], [a[0]], w.keys)
    got = bank.select_result(0, 2)
    words = w.assemble(second, {**host_sources(cts), (2, 0): old})
    assert np.array_equal(got[0], w.oselect(2, words, w.index_digits(0, 2)))
    assert np.array_equal(got[1], w.oselect(2, words[1:], w.index_digits(0, 2)))
    ref.write(got[0:1], [a[0]], w.keys, first=0)
    assert np.array_equal(bank.store_encrypted(0), ref.store_encrypted(0)) and bank.state(0) is False
    back = bank.read([a[0]], w.keys, first=0)[0]
    w.check_value(back, [w.data[0][0 + 4 * w.idx[0]], vals[2][0], w.data[0][2 + 4 * w.idx[0]], w.data[0][3 + 4 * w.idx[0]]], "SB at offset 1")


# ---- 6. field selectors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [[2, 2], [1, 3], [2, 3]], ids=["2_2", "1_3", "2_3"])
def test_field_selectors_equal_the_oracle(w4, bank4, widths):
    """digits from two integers at first bits 0, 7 and 30, derived in place over fheram_bank_selector_create_fields and over an earlier
    derivation; a select through each"""
    w, pkg = w4, w4.pkg
    bank = bank4
    fa, fb = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE)), pkg.FheUintPrepared.from_host(bank, w.bits(VALUE_B))
    bits = sum(widths)
    m = min(1 << bits, 20)
    vals, cts = w.candidates(20, seed=60)
    made = pkg.Selector.from_digits_fields(bank, widths, list(w.field_digits(widths, (VALUE_B, VALUE), (3, 11))))
    assert made.n_digits() == len(widths) == 2 and made.bits == bits
    assert np.array_equal(made.download(), w.field_digits(widths, (VALUE_B, VALUE), (3, 11)))
    fresh = bank.selector_fields(widths)
    bank.profile_reset()
    bank.profile_enable(True)
    bank.derive_selector_fields(fresh, [fa, fb], [0, 7])
    bank.sync()
    prof = bank.profile_get("derive")
    bank.profile_enable(False)
    assert prof["launches"] == 2 and prof["blocks"] == 2 * 6, prof   # one launch of grid (6, 1, 1) per field
    for sel, firsts in ((fresh, (0, 7)), (made, (7, 0)), (fresh, (30, 7))):   # over _alloc_fields / _create_fields / an earlier derivation
        bank.derive_selector_fields(sel, [fa, fb], list(firsts))
        digits = w.field_digits(widths, (VALUE, VALUE_B), firsts)
        assert np.array_equal(sel.download(), digits), (widths, firsts)
        index = sum((((v >> f) & ((1 << wd) - 1)) << lsh) for v, f, wd, lsh in zip((VALUE, VALUE_B), firsts, widths, (0, widths[0])))
        got = bank.select([sel], [host_srcs(pkg, m)], host_words=cts)[0]
        assert np.array_equal(got, w.oselect_fields(widths, cts[:m], digits)), (widths, firsts)
        noise = w.check_value(got, vals[index] if index < m else None, (widths, firsts, index))
        print(f"field selector {widths} first bits {firsts} index {index}: log2 noise {noise:.2f}")
    # the same integer for both fields, and a lanes select through a field selector
    bank.derive_selector_fields(made, [fa, fa], [4, 20])
    digits = w.field_digits(widths, (VALUE, VALUE), (4, 20))
    assert np.array_equal(made.download(), digits)
    cands = [[pkg.Lane.host(j, 3 - wd) for wd in range(4)] for j in range(m)]
    got = bank.select_lanes([made], [cands], host_words=cts)[0]
    assert np.array_equal(got, w.oselect_fields(widths, w.assemble(cands, host_sources(cts)), digits))


def test_mixed_digit_counts_are_refused_and_equal_ones_share_a_call(w4, bank4):
    w, pkg = w4, w4.pkg
    bank = bank4
    vals, cts = w.candidates(20, seed=60)
    d22 = w.field_digits([2, 2], (VALUE, VALUE_B), (0, 7))
    f22 = pkg.Selector.from_digits_fields(bank, [2, 2], list(d22))
    f13 = pkg.Selector.from_digits_fields(bank, [1, 3], list(w.field_digits([1, 3], (VALUE, VALUE_B), (0, 7))))
    plain4 = w.selector(bank, 9, 4)   # the bank's own plan for 4 bits: [3, 1], two digits too
    plain3 = w.selector(bank, 5, 3)   # [3]: one digit
    f111 = bank.selector_fields([1, 1, 1])
    bank.derive_selector_fields(f111, [pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))] * 3, [0, 1, 2])
    srcs = host_srcs(pkg, 8)
    with pytest.raises(pkg.FheRamError) as e:   # 3 bits in three digits beside 3 bits in one
        bank.select([plain3, f111], [srcs] * 2, host_words=cts)
    assert e.value.code == ST_INVALID_ARG and "digits" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:   # the existing check stays first, with its message
        bank.select([f22, plain3], [srcs] * 2, host_words=cts)
    assert e.value.code == ST_INVALID_ARG and "bits" in e.value.msg and "digit count" in e.value.msg
    with pytest.raises(pkg.FheRamError) as e:
        bank.select_lanes([f111, plain3], [[[pkg.Lane.host(0, wd) for wd in range(4)]]] * 2, host_words=cts)
    assert e.value.code == ST_INVALID_ARG and "digits" in e.value.msg
    # [2, 2], [1, 3] and the bank's [3, 1] have 4 bits in two digits: one call, each read with its own plan
    got = bank.select([f22, f13, plain4], [host_srcs(pkg, 16)] * 3, host_words=cts)
    assert np.array_equal(got[0], w.oselect_fields([2, 2], cts[:16], d22))
    assert np.array_equal(got[1], w.oselect_fields([1, 3], cts[:16], w.field_digits([1, 3], (VALUE, VALUE_B), (0, 7))))
    assert np.array_equal(got[2], w.oselect(4, cts[:16], w.index_digits(9, 4)))
    got = bank.select([f111], [srcs], host_words=cts)[0]   # three one-bit digits from bits 0, 1, 2 of VALUE
    assert np.array_equal(got, w.oselect_fields([1, 1, 1], cts[:8], w.field_digits([1, 1, 1], (VALUE,) * 3, (0, 1, 2))))
    w.check_value(got, vals[VALUE & 7], "three fields")


# ---- 7. addresses from a bit offset ---------------------------------------------------------------------------------------------------------
def test_derive_at(w2):
    """on a context (whose address digits can be downloaded): first_bit 0 is derive, 2 and 18 against the oracle on the integer's bits from there
    on, two offsets in one call, in place, refusals; on a bank: the reads through such addresses"""
    w, pkg = w2, w2.pkg

    def want(value, f):
        return w.o.address_from_fheuint(w.bits(value)[f:], sign=False)

    def digits(addr):
        return np.stack(addr.digits)

    ram = w.new_ram(1)
    fu = pkg.FheUintPrepared.from_host(ram, w.bits(VALUE))
    fb = pkg.FheUintPrepared.from_host(ram, w.bits(VALUE_B))
    plain = ram.derive_addresses([fu])[0]
    at0 = ram.derive_addresses([fu], first_bits=[0])[0]
    assert np.array_equal(digits(at0), digits(plain)) and np.array_equal(digits(at0), want(VALUE, 0))
    ram.profile_enable(True)
    a2, a18, b2 = ram.derive_addresses([fu, fu, fb], first_bits=[2, 18, 2])   # two launches: two distinct first bits
    ram.sync()
    prof = ram.profile_get("derive")
    ram.profile_enable(False)
    assert prof["launches"] == 2 and prof["blocks"] == 3 * 6 * 4, prof
    assert np.array_equal(digits(a2), want(VALUE, 2))
    assert np.array_equal(digits(a18), want(VALUE, 18))
    assert np.array_equal(digits(b2), want(VALUE_B, 2))
    ram.derive_addresses([fb, fu], addrs=[a2, at0], first_bits=[20, 5])   # in place, over earlier derivations
    assert np.array_equal(digits(a2), want(VALUE_B, 20)) and np.array_equal(digits(at0), want(VALUE, 5))
    before = sha(digits(a18))
    for firsts in ([21], [-1], [32]):
        with pytest.raises(pkg.FheRamError) as e:
            ram.derive_addresses([fu], addrs=[a18], first_bits=firsts)
        assert e.value.code == ST_INVALID_ARG, firsts
    with pytest.raises(pkg.FheRamError) as e:   # the whole list is checked before anything is enqueued
        ram.derive_addresses([fu, fu], addrs=[a18, a2], first_bits=[3, 21])
    assert e.value.code == ST_INVALID_ARG
    a18._digits = None
    assert sha(digits(a18)) == before
    # the bank's entry point: a derived address reads the word at bits [2, 14) of the integer, two offsets in one call
    bank = w.new_bank(3)
    bfu = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))
    c2, c18 = bank.derive_addresses([bfu, bfu], first_bits=[2, 18])
    got = bank.read_list([1, 2], [c2, c18], w.keys)
    assert np.array_equal(got[0], w.new_oram(1).read(w.o.address_new(want(VALUE, 2)), w.okeys))
    assert np.array_equal(got[1], w.new_oram(2).read(w.o.address_new(want(VALUE, 18)), w.okeys))
    idx = (VALUE >> 2) & 0xFFF
    for i in range(w.ws):
        plain_i = w.o.expected_plain(int(w.data[1][i + w.ws * idx]), w.o.p.k_glwe_pt)
        assert w.o.glwe_decrypt(got[0][i], plain_i, w.sk)[0] == plain_i
    with pytest.raises(pkg.FheRamError) as e:
        bank.derive_addresses([bfu], addrs=[c2], first_bits=[21])
    assert e.value.code == ST_INVALID_ARG
    assert np.array_equal(bank.read([c2], w.keys, first=1)[0], got[0]), "a refused call changed the address"


# ---- 8. end to end at 2^13: a byte-addressed store and load ---------------------------------------------------------------------------------
WORD = 0x0B5E   # the word address: bits [2, 15) of the byte address
DATA, REGS = 2, 0   # the data memory and the register file
_E2E = {}


def e2e_setup(w):
    """what every case shares: x = the register word (a read-list entry of member REGS), per offset the oracle's address and old word"""
    if id(w) not in _E2E:
        x = w.new_oram(REGS).read(w.o.address_new(w.addr_g[1]), w.okeys)
        _E2E[id(w)] = {"x": x, "xbytes": [int(w.data[REGS][i + 4 * w.idx[1]]) for i in range(4)],
                       "ybytes": [int(w.data[DATA][i + 4 * WORD]) for i in range(4)], "offset": {}}
    return _E2E[id(w)]


def e2e_offset(w, offset):
    s = e2e_setup(w)
    if offset not in s["offset"]:
        byte_addr = (WORD << 2) | offset
        digits = w.o.address_from_fheuint(w.bits(byte_addr)[2:], sign=False)
        old = w.new_oram(DATA).read_prepare_write(w.o.address_new(digits), w.okeys)
        s["offset"][offset] = (byte_addr, digits, old)
    return s["offset"][offset]


def word_of(bs):
    return sum(b << (8 * i) for i, b in enumerate(bs))


def e2e_run(w, cands_of, op, offset, y_from_read):
    """one step on the device, with no download in between: address from bits [2, ..) of the byte address, the [2, 2] selector from `op` and
    the address's low bits, select_lanes, write_list_selected; returns (bank, x, y, target member, address digits)"""
    pkg, S = w.pkg, w.pkg.Src
    byte_addr, digits, old = e2e_offset(w, offset)
    bank = w.new_bank(3)
    fu_addr = pkg.FheUintPrepared.from_host(bank, w.bits(byte_addr))
    fu_op = pkg.FheUintPrepared.from_host(bank, w.bits(op))
    sel = bank.selector_fields([2, 2])
    addr = bank.derive_addresses([fu_addr], first_bits=[2])[0]
    bank.derive_selector_fields(sel, [fu_op, fu_addr], [0, 0])
    if y_from_read:   # a load: the data word is read, the register file takes the extracted word
        bank.read_list([DATA], [addr], w.keys, download=False)
        bank.read_prepare_write([w.addrs[1]], w.keys, first=REGS, download=False)
        bank.select_lanes([sel], [cands_of(S.list(0))], download=False)
        bank.write_list_selected([REGS], [0], [w.addrs[1]], w.keys)
    else:             # a store: the register word is read, the data memory takes the merged word
        bank.read_list([REGS], [w.addrs[1]], w.keys, download=False)
        bank.read_prepare_write([addr], w.keys, first=DATA, download=False)
        bank.select_lanes([sel], [cands_of(S.list(0), S.member(DATA))], download=False)
        bank.write_list_selected([DATA], [0], [addr], w.keys)
    return bank, addr, digits, old


STORES = [(offset, op) for offset in range(4) for op in range(4) if op < 2 or (op == 2 and offset in (0, 2)) or (op == 3 and offset == 0)]


@pytest.mark.parametrize("offset,op", STORES)
def test_store_merge_end_to_end(w13, offset, op):
    """every valid (offset, op) of the store merge: rows and a read-back equal oracle Rams given the oracle-selected word, and the bytes are the
    reference test's c_want"""
    w, pkg = w13, w13.pkg
    s = e2e_setup(w)
    bank, addr, digits, old = e2e_run(w, lambda x, y: pkg.store_merge_lanes(x, y), op, offset, False)
    cands = pkg.store_merge_lanes(pkg.Src.list(0), pkg.Src.member(DATA))
    words = w.assemble(cands, {(3, 0): s["x"], (2, DATA): old})
    sel_digits = w.field_digits([2, 2], (op, (WORD << 2) | offset), (0, 0))
    pick = w.oselect_fields([2, 2], words, sel_digits)
    assert np.array_equal(bank.select_result(0, 1)[0], pick), (offset, op)
    assert np.array_equal(bank.list_result(0, 1)[0], s["x"]) and np.array_equal(bank.result(DATA, 1)[0], old)
    oram, oa = w.new_oram(DATA), w.o.address_new(digits)
    oram.read_prepare_write(oa, w.okeys)
    oram.write(pick, oa, w.okeys)
    assert np.array_equal(np.ravel(bank.store_encrypted(DATA)), np.ravel(oram.store())), (offset, op, "rows")
    assert np.array_equal(bank.tree(DATA, 0), oram.tree(0)) and bank.state(DATA) is False
    back = bank.read([addr], w.keys, first=DATA)[0]
    assert np.array_equal(back, oram.read(oa, w.okeys)), (offset, op, "read-back")
    want = c_want(word_of(s["xbytes"]), word_of(s["ybytes"]), offset, op)
    noise = w.check_value(back, [(want >> (8 * i)) & 0xFF for i in range(4)], (offset, op))
    print(f"store offset={offset} op={op}: log2 noise of the read-back {noise:.2f}")
    for m in (REGS, 1):
        assert np.array_equal(np.ravel(bank.store_encrypted(m)), np.ravel(w.rows[m])), "a member that was not written changed"


def test_load_extract_end_to_end(w13):
    """LHU at offset 2: the data word's upper half, zero-extended, lands in the register file"""
    w, pkg = w13, w13.pkg
    offset, op = 2, 2
    s = e2e_setup(w)
    bank, addr, digits, _ = e2e_run(w, lambda y: pkg.load_extract_lanes(y), op, offset, True)
    y = w.new_oram(DATA).read(w.o.address_new(digits), w.okeys)
    assert np.array_equal(bank.list_result(0, 1)[0], y)
    words = w.assemble(pkg.load_extract_lanes(pkg.Src.list(0)), {(3, 0): y})
    pick = w.oselect_fields([2, 2], words, w.field_digits([2, 2], (op, (WORD << 2) | offset), (0, 0)))
    assert np.array_equal(bank.select_result(0, 1)[0], pick)
    oram, oa = w.new_oram(REGS), w.o.address_new(w.addr_g[1])
    oram.read_prepare_write(oa, w.okeys)
    oram.write(pick, oa, w.okeys)
    assert np.array_equal(np.ravel(bank.store_encrypted(REGS)), np.ravel(oram.store()))
    back = bank.read([w.addrs[1]], w.keys, first=REGS)[0]
    assert np.array_equal(back, oram.read(oa, w.okeys))
    noise = w.check_value(back, [s["ybytes"][2], s["ybytes"][3], 0, 0], "LHU at offset 2")
    print(f"load LHU offset=2: log2 noise of the read-back {noise:.2f}")


# ---- 9. forced forms -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [{"safe": 1}, {"tail": 0}, {"fuse": 0}, {"memo": 0}], ids=["safe", "tail0", "fuse0", "memo0"])
def test_forced_forms_give_the_same_integers(w4, bank4, config):
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    b, m = 5, 20
    vals, cts = w.candidates(20, seed=60)
    cands = [[L.host((j + wd) % m, (2 * wd + j) % 4) for wd in range(4)] for j in range(m)]
    bank = w.new_bank(3, config=config)
    bank._use_keys(w.keys)
    for idx, n in ((10, 1), (19, 3)):   # one select (no table of operands) and three
        want = bank4.select_lanes([w.selector(bank4, idx, b)], [cands], host_words=cts)[0]
        got = bank.select_lanes([w.selector(bank, idx, b)] * n, [cands] * n, host_words=cts)
        for k in range(n):
            assert np.array_equal(got[k], want), (config, idx, k, np.count_nonzero(got[k] != want))
    assert bank.roundoff_max() < 0.375


# ---- 10. launch profile ----------------------------------------------------------------------------------------------------------------------
def test_launch_profile(w4, bank4):
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    vals, cts = w.candidates(20, seed=60)
    for n, b, m in ((1, 5, 20), (4, 5, 20), (3, 1, 2)):
        sels = [w.selector(bank4, k, b) for k in range(n)]
        cands = [[L.host(j, 3 - wd) for wd in range(4)] for j in range(m)]
        bank4.sync()
        bank4.profile_reset()
        bank4.profile_enable(True)
        bank4.select_lanes(sels, [cands] * n, host_words=cts)
        prof = bank4.profile_get("select_pack")
        bank4.profile_enable(False)
        assert prof["launches"] == 1 and prof["blocks"] == n * w.ws, (n, b, m, prof)


# ---- 11. refusals: all host-side, before anything is enqueued --------------------------------------------------------------------------------
def test_refusals_change_nothing(w4, w2):
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    lb = lib()
    vals, cts = w.candidates(3)
    bank = w.new_bank(3)
    other = w2.new_bank(1)
    fresh = w.new_bank(3)   # keys not loaded, nothing run
    bank.read([w.addrs[0]], w.keys, first=0)
    bank.read_list([1, 0], [w.addrs[1], w.addrs[2]], w.keys)
    sel = w.selector(bank, 1, 2)
    foreign = w2.selector(other, 1, 2)
    fu = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))
    fu10 = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE)[:10])
    fu_other = pkg.FheUintPrepared.from_host(other, w2.bits(VALUE))
    fsel = pkg.Selector.from_digits_fields(bank, [1, 1], list(w.field_digits([2, 2], (VALUE, VALUE_B), (0, 7))))   # (any two digits)

    def digest():
        return ([sha(bank.store_encrypted(m)) for m in range(3)], [bank.state(m) for m in range(3)], sha(bank.result(0, 3)), sha(bank.list_result(0, 2)),
                sha(sel.download()), sha(fsel.download()))

    before = digest()

    def refused(code, call, what):
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg, what

    word = lambda i: [L.host(i, wd) for wd in range(4)]   # noqa: E731
    ok = [word(0), word(1), word(2)]
    # -- select_lanes: the refusals of select ...
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([bank.selector(2)], [ok], host_words=cts), "underived selector")
    refused(ST_INVALID_ARG, lambda: other.select_lanes([sel], [[[L.host(0, 0), L.host(0, 1)]]], host_words=cts), "selector of another bank")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [ok + [word(0), word(1)]], host_words=cts), "n_cand > 2^bits")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L(9, 0, 0)] * 4]], host_words=cts), "unknown source kind")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L.member(3, 0)] * 4]]), "member outside the bank")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L.list_entry(2, 0)] * 4]]), "entry outside the last list")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[word(0)]]), "HOST without host_words")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel] * 9, [ok] * 9, host_words=cts), "n = 9")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel, w.selector(bank, 0, 1)], [ok[:2]] * 2, host_words=cts), "mixed bits")
    # ... and its own
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L.host(0, 0), L.host(0, 1), L.host(0, 2), L.host(0, 4)]]], host_words=cts), "lane = word_size")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L.member(0, -1)] * 4]]), "negative lane")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L(1, 0, 0, reserved=1)] * 4]], host_words=cts), "reserved != 0")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L(0, 0, 0, reserved=7)] * 4]]), "reserved != 0 on a ZERO lane")
    n_cand, p1 = (C.c_int * 1)(1), (C.c_void_p * 1)(sel._h)
    lane4 = (pkg.api._CSelectLane * 4)(*[pkg.api._CSelectLane(0, 0, 99, 0)] * 4)   # ZERO: the lane is ignored
    assert lb.fheram_bank_select_lanes(bank._h, None, n_cand, 1, lane4, None, None) == ST_INVALID_ARG
    assert lb.fheram_bank_select_lanes(bank._h, p1, None, 1, lane4, None, None) == ST_INVALID_ARG
    assert lb.fheram_bank_select_lanes(bank._h, p1, n_cand, 1, None, None, None) == ST_INVALID_ARG
    assert lb.fheram_bank_select_lanes(bank._h, p1, n_cand, 0, lane4, None, None) == ST_INVALID_ARG
    refused(ST_STATE, lambda: bank.select_lanes([sel], [[[L.member(2, 0)] * 4]]), "a member without a result")
    refused(ST_STATE, lambda: bank.select_lanes([sel], [[[L.select(0, 0)] * 4]]), "no select has run")
    bad = cts.copy()
    bad[1, 2, 5] = (1 << 16) + 1
    refused(ST_RANGE, lambda: bank.select_lanes([sel], [ok], host_words=bad), "host limb out of range")
    fs = w.selector(fresh, 1, 2)
    refused(ST_KEYS, lambda: fresh.select_lanes([fs], [ok], host_words=cts), "keys not loaded")
    refused(ST_STATE, lambda: fresh.select_lanes([fs], [[[L.list_entry(0, 0)] * 4]], keys=w.keys), "no read list has run")
    # -- field selectors
    refused(ST_INVALID_ARG, lambda: bank.selector_fields([]), "no field")
    refused(ST_INVALID_ARG, lambda: bank.selector_fields([1] * 6), "six fields")
    refused(ST_INVALID_ARG, lambda: bank.selector_fields([2, 0]), "a width of 0")
    refused(ST_INVALID_ARG, lambda: bank.selector_fields([3, 3]), "six bits")
    refused(ST_INVALID_ARG, lambda: pkg.Selector.from_digits_fields(bank, [2, 2], list(fsel.download())[:1]), "n_ggsw != n_fields")
    refused(ST_INVALID_ARG, lambda: bank.derive_selector_fields(fsel, [fu, fu_other], [0, 0]), "integer of another bank")
    refused(ST_INVALID_ARG, lambda: other.derive_selector_fields(fsel, [fu_other, fu_other], [0, 0]), "selector of another bank")
    refused(ST_INVALID_ARG, lambda: bank.derive_selector_fields(fsel, [fu, fu], [0, 32]), "a field beyond the integer")
    refused(ST_INVALID_ARG, lambda: bank.derive_selector_fields(fsel, [fu, fu10], [0, 10]), "a field beyond a narrow integer")
    refused(ST_INVALID_ARG, lambda: bank.derive_selector_fields(fsel, [fu, fu], [-1, 0]), "negative first bit")
    refused(ST_INVALID_ARG, lambda: bank.derive_selectors([fu], [0], [fsel]), "derive_selectors on a field selector")
    two_i, two_p = (C.c_int * 2)(0, 0), (C.c_void_p * 2)(fu._h, fu._h)
    assert lb.fheram_bank_selector_derive_fields(bank._h, sel._h, two_p, two_i) == ST_INVALID_ARG   # not made by a _fields call
    assert lb.fheram_bank_selector_derive_fields(bank._h, None, two_p, two_i) == ST_INVALID_ARG
    assert lb.fheram_bank_selector_derive_fields(bank._h, fsel._h, None, two_i) == ST_INVALID_ARG
    assert lb.fheram_bank_selector_derive_fields(bank._h, fsel._h, two_p, None) == ST_INVALID_ARG
    assert lb.fheram_bank_selector_alloc_fields(bank._h, None, 2, C.byref(C.c_void_p())) == ST_INVALID_ARG
    assert lb.fheram_bank_selector_alloc_fields(bank._h, two_i, 2, None) == ST_INVALID_ARG
    assert digest() == before
    # ... in a ciphertext no lane names: not looked at; and the bank still selects
    got = bank.select_lanes([sel], [[word(0), [L.host(1, 0), L.host(1, 1), L.host(1, 3), L.host(1, 3)]]], host_words=bad)[0]
    words = w.assemble([[L.host(1, 0), L.host(1, 1), L.host(1, 3), L.host(1, 3)]], host_sources(cts))
    assert np.array_equal(got, w.oselect(2, np.concatenate([cts[0:1], words]), w.index_digits(1, 2)))
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[L.select(1, 0)] * 4]]), "output outside the last select")


def test_table_allocation_failure_is_reported_and_the_next_call_works(w4):
    """the pointer table is allocated on the first lanes call, behind the select's own buffers: the self-test's failing allocation reaches it as
    the one after those (include/fheram.h); nothing is kept of the failure, plain selects never notice, and the next lanes call works"""
    w, pkg, L = w4, w4.pkg, w4.pkg.Lane
    vals, cts = w.candidates(3)
    bank = w.new_bank(3)
    bank._use_keys(w.keys)
    sel = w.selector(bank, 1, 1)
    cands = [[L.host(0, 3 - wd) for wd in range(4)], [L.host(1, 3 - wd) for wd in range(4)]]
    want = w.oselect(1, w.assemble(cands, host_sources(cts)), w.index_digits(1, 1))
    plain = bank.select([sel], [host_srcs(pkg, 2)], host_words=cts)[0]   # the select's buffers exist now: the table's is the next allocation
    bank.selftest_fail_select_alloc(1)
    with pytest.raises(pkg.FheRamError) as e:
        bank.select_lanes([sel], [cands], host_words=cts)
    assert e.value.code == ST_DEVICE, e.value
    assert np.array_equal(bank.select_result(0, 1)[0], plain), "the last select's output is still there"
    assert np.array_equal(bank.select([sel], [host_srcs(pkg, 2)], host_words=cts)[0], plain)
    assert np.array_equal(bank.select_lanes([sel], [cands], host_words=cts)[0], want)
    bank.selftest_fail_select_alloc(1)   # the table exists: a lanes call that fits allocates nothing, the request stays pending for the next growth
    assert np.array_equal(bank.select_lanes([sel], [cands], host_words=cts)[0], want)
    with pytest.raises(pkg.FheRamError) as e:
        bank.select_lanes([sel] * 2, [cands] * 2, host_words=cts)
    assert e.value.code == ST_DEVICE
    got = bank.select_lanes([sel] * 2, [cands] * 2, host_words=cts)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
