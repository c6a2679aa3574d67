"""fheram_bank_table_* (RamBank.table, Table, RamBank.table_read / table_selector): a bank's tables — read-only one-row RAMs of 2^bits words,
bits <= 12, that live beside the members and the register files and are read at WIDE selectors (include/fheram.h).

The contract, in the oracle's own operations: with ob = Oracle(OParams(max_addr = 2^b, word_size = ws)) (SelWorld.small(b)) and its one-row
RAM, entry k of RamBank.table_read is ORam.read at address_new(selector digits) of the row tables[k] holds.  Every comparison is
np.array_equal on int64; the noise of a decrypted output is printed, not bounded.  Banks are at max_addr = 2^12 (one
row, one coordinate) with 2 members and word_size = 2; the worlds and helpers are test_gpu_regs.py's."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import World, lib, sha
from test_gpu_regs import (bank2, decrypts_to, enc_digits, oaddr, oram_of, orow, regs_rows, w2, word_of)  # noqa: F401 (w2, bank2: fixtures)
from test_gpu_regs import selector as narrow_selector
from test_gpu_select import VALUE, SelWorld

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS, ST_UNSUPPORTED, ST_RANGE = 1, 2, 3, 4, 5, 6
I64P, U8P = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
VALUE_B = 0x4A1C5926   # a second encrypted integer: the field selector takes its fields from two
PLANS = {6: [3, 3], 7: [3, 3, 1], 9: [3, 3, 3], 10: [3, 3, 3, 1], 12: [3, 3, 3, 3]}


def wide(w, bank, idx, b):
    """the wide selector of index idx of a table of b bits, from freshly encrypted host digits"""
    return bank.table_selector(b, list(enc_digits(w, idx, b)))


def loaded_table(w, bank, b, seed=0):
    data, row = regs_rows(w, b, seed)
    t = bank.table(b)
    t.load(row)
    return t, data, row


def oracle_reads(w, b, row, idxs):
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    return [oram.read(oaddr(w, i, b), okeys) for i in idxs]


# ---- 1. reads at the plan boundaries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [6, 7, 9, 12])
def test_read_equals_the_oracle(w2, bank2, b):
    """the plans [3,3], [3,3,1], [3,3,3] and [3,3,3,3]: two digits, a ragged last digit, and the four the tail fuses; index 0, 2^b - 1 and a
    middle one in ONE call, one selector twice; the row does not change"""
    w = w2
    assert w.po.get_base_2d(1 << b, [3, 3, 3, 3]) == [PLANS[b]] and w.small(b)[0].n_digits == len(PLANS[b])
    t, data, row = loaded_table(w, bank2, b)
    assert t.bits == b and lib().fheram_table_bits(t._h) == b
    assert np.array_equal(t.download(), row)
    idxs = [0, (1 << b) - 1, (1 << b) // 2 + 5]
    sels = [wide(w, bank2, i, b) for i in idxs]
    assert all(s.n_digits() == len(PLANS[b]) for s in sels)
    sels.append(sels[1])
    idxs.append(idxs[1])
    got = bank2.table_read([t] * 4, sels)
    assert got.shape == (4, w.ws, w.params.glwe_len())
    for k, (idx, want) in enumerate(zip(idxs, oracle_reads(w, b, row, idxs))):
        assert np.array_equal(got[k], want), (b, k, idx, np.count_nonzero(got[k] != want))
        noise = decrypts_to(w, got[k], word_of(w, data, idx), False, (b, idx))
        print(f"table read b={b} idx={idx}: log2 noise {noise:.2f}")
    assert sha(t.download()) == sha(row), "a read changed the table"
    assert bank2.table_read([t, t], sels[:2], download=False) is None
    assert np.array_equal(bank2.table_result(0, 2), got[:2]) and np.array_equal(bank2.table_result(1, 1)[0], got[1])


# ---- 2. two tables in one call ------------------------------------------------------------------------------------------------------------------
def test_two_tables_in_one_call(w2, bank2):
    """12 and 10 bits are both four digits ([3,3,3,3], [3,3,3,1]): one call reads both, each entry as its single-table call; 12 beside 9 bits
    (three digits) is refused"""
    w = w2
    t12, d12, r12 = loaded_table(w, bank2, 12)
    t10, d10, r10 = loaded_table(w, bank2, 10)
    t9, d9, r9 = loaded_table(w, bank2, 9)
    s12, s10, s9 = wide(w, bank2, 3001, 12), wide(w, bank2, 777, 10), wide(w, bank2, 300, 9)
    assert s12.n_digits() == s10.n_digits() == 4 and s9.n_digits() == 3
    got = bank2.table_read([t12, t10, t12], [s12, s10, s12])
    one12, one10 = bank2.table_read([t12], [s12])[0], bank2.table_read([t10], [s10])[0]
    assert np.array_equal(got[0], one12) and np.array_equal(got[1], one10) and np.array_equal(got[2], one12)
    assert np.array_equal(one12, oracle_reads(w, 12, r12, [3001])[0]) and np.array_equal(one10, oracle_reads(w, 10, r10, [777])[0])
    decrypts_to(w, got[1], word_of(w, d10, 777), False, "the 10-bit table")
    before = sha(bank2.table_result(0, 1))
    with pytest.raises(w.pkg.FheRamError) as e:
        bank2.table_read([t12, t9], [s12, s9])
    assert e.value.code == ST_INVALID_ARG and "digits" in e.value.msg, e.value
    assert sha(bank2.table_result(0, 1)) == before and sha(t9.download()) == sha(r9)


# ---- 3. configurations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [{"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}], ids=["safe_monitor2", "tail0_fuse0"])
def test_read_under_other_configurations(w2, bank2, config):
    """the bits-12 read under `safe` with the monitor on every launch, and without the tail launch and the fused products: the same int64, no
    FHERAM_ERR_PRECISION"""
    w = w2
    b, idxs = 12, [0, 4095, 2053]
    bank = w.new_bank(2, config=config)
    bank._use_keys(w.keys)
    t, data, row = loaded_table(w, bank, b)
    got = bank.table_read([t] * 3, [wide(w, bank, i, b) for i in idxs])
    t0, _, _ = loaded_table(w, bank2, b)
    default = bank2.table_read([t0] * 3, [wide(w, bank2, i, b) for i in idxs])
    assert np.array_equal(got, default), np.count_nonzero(got != default)
    for k, want in enumerate(oracle_reads(w, b, row, idxs)):
        assert np.array_equal(got[k], want), (config, k)
    print(f"table read {config}: round-off maximum {bank.roundoff_max():.4f}")   # (raises FHERAM_ERR_PRECISION above 3/8)


# ---- 4. load_plain --------------------------------------------------------------------------------------------------------------------------------
class _Zeros:
    """mask and noise sources that draw zeros: Ram::encrypt_sk then gives the trivial ciphertext"""

    def uniform_limbs(self, count):
        return np.zeros(count, dtype=np.int64)

    def gaussian(self, count, scale):
        return np.zeros(count, dtype=np.int64)


@pytest.mark.parametrize("b", [7, 12])
def test_load_plain_is_the_trivial_encryption(w2, bank2, b):
    """b = 7 leaves coefficients [128, 4096) zero padding; b = 12 fills the row"""
    w, pkg = w2, w2.pkg
    p = w.params
    data = np.random.default_rng(7600 + b).integers(0, 256, size=(1 << b) * w.ws, dtype=np.uint8)
    t = bank2.table(b)
    t.load_plain(data)
    row = t.download()
    limbs = row.reshape(w.ws, -1, 2, p.n())   # [ws][limb][column][N]
    assert not np.any(limbs[:, :, 1, :]), "a mask limb is not zero"
    ram = pkg.Ram.new_from_ram_params(w.ws, [3, 3, 3, 3], 1 << b)
    ram.encrypt_sk(data, pkg.GLWESecret(ram, w.sk), _Zeros(), _Zeros())
    want = ram.store_encrypted().reshape(w.ws, -1)
    assert np.array_equal(row, want), np.count_nonzero(row != want)
    for coeff in (0, 1, (1 << b) - 1):
        for i in range(w.ws):
            plain = w.o.expected_plain(int(data[i + w.ws * coeff]), w.o.p.k_glwe_pt, False)
            v, _ = w.o.glwe_decrypt(row[i], plain, w.sk, coeff)
            assert v == plain, (b, coeff, i, v, plain)
    idxs = [0, (1 << b) - 1, (1 << b) // 3]
    got = bank2.table_read([t] * 3, [wide(w, bank2, i, b) for i in idxs])
    for k, (idx, ref) in enumerate(zip(idxs, oracle_reads(w, b, row, idxs))):
        assert np.array_equal(got[k], ref), (b, idx)
        noise = decrypts_to(w, got[k], word_of(w, data, idx), False, ("plain", b, idx))
        print(f"plain table read b={b} idx={idx}: log2 noise {noise:.2f}")
    # a second load straight behind the first (the staging buffer's one wait), then the first contents again
    t.load_plain(data[::-1].copy())
    t.load_plain(data)
    assert sha(t.download()) == sha(row)


# ---- 5. wide selectors ------------------------------------------------------------------------------------------------------------------------------
def test_fetch_index_and_rs1_from_one_derive_list(w2, bank2):
    """the fetch index = bits [2, 14) of the pc and a 5-bit rs1 = bits [15, 20) in ONE launch; the digits equal fheram_bank_selector_derive's and
    the oracle's, and the ROM reads the instruction"""
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    b = 12
    fu = pkg.FheUintPrepared.from_host(bank2, w.bits(VALUE))
    fetch, alone, rs1 = bank2.table_selector(b), bank2.table_selector(b), bank2.selector(5)
    assert fetch.n_digits() == 4
    bank2.profile_enable(True)
    bank2.profile_reset()
    bank2.derive_list([D.selector(fu, fetch, 2), D.selector(fu, rs1, 15)])
    bank2.sync()
    prof = bank2.profile_get("derive")
    bank2.profile_enable(False)
    assert prof["launches"] == 1 and prof["blocks"] == 6 * (4 + 2), prof
    bank2.derive_selectors([fu], [2], [alone])
    want = w.digits(VALUE, 2, b)
    assert np.array_equal(fetch.download(), want) and np.array_equal(alone.download(), want)
    assert np.array_equal(rs1.download(), w.digits(VALUE, 15, 5))
    t, data, row = loaded_table(w, bank2, b)
    got = bank2.table_read([t], [fetch])[0]
    ob, okeys = w.small(b)
    assert np.array_equal(got, oram_of(w, b, row).read(ob.address_new(want), okeys))
    noise = decrypts_to(w, got, word_of(w, data, (VALUE >> 2) & 4095), False, "the fetched word")
    print(f"table fetch at a derived index {(VALUE >> 2) & 4095}: log2 noise {noise:.2f}")


def test_field_selector_of_two_six_bit_fields(w2, bank2):
    """widths (6, 6): the Address of an oracle whose DECOMP_N is [6, 6]; digit 0 from bits [3, 9) of one integer, digit 1 from bits [11, 17) of
    another, through the derive list and through fheram_bank_selector_derive_fields"""
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    assert w.po.get_base_2d(1 << 12, [6, 6]) == [[6, 6]]
    ob = w.po.Oracle(w.oparams(1 << 12, decomp_n=[6, 6]))
    okeys = ob.keys_prepare(w.evk)
    fa, fb = (pkg.FheUintPrepared.from_host(bank2, w.bits(v)) for v in (VALUE, VALUE_B))
    digits = ob.address_from_fheuint(np.concatenate([w.bits(VALUE)[3:9], w.bits(VALUE_B)[11:17]]), sign=False)
    f, g = bank2.table_selector_fields([6, 6]), bank2.table_selector_fields([6, 6])
    assert f.n_digits() == 2 and f.bits == 12
    bank2.derive_list([D.fields(f, [fa, fb], [3, 11])])
    bank2.derive_selector_fields(g, [fa, fb], [3, 11])
    assert np.array_equal(f.download(), digits) and np.array_equal(g.download(), digits)
    t, data, row = loaded_table(w, bank2, 12)
    got = bank2.table_read([t], [f])[0]
    oram = ob.ram_new()
    oram.load(row.reshape(w.ws, 1, -1))
    assert np.array_equal(got, oram.read(ob.address_new(digits), okeys))
    index = ((VALUE >> 3) & 63) | (((VALUE_B >> 11) & 63) << 6)
    noise = decrypts_to(w, got, word_of(w, data, index), False, "the word at the two fields")
    print(f"table read at a (6, 6) field selector, index {index}: log2 noise {noise:.2f}")


# ---- 6. other DECOMP_N -----------------------------------------------------------------------------------------------------------------------------
class PlanWorld(SelWorld):
    """a SelWorld over another DECOMP_N, the small oracles too"""

    def __init__(self, po, plan, seed):
        World.__init__(self, po, 1 << 12, 2, word_size=2, seed=seed, n_addr=3, decomp_n=list(plan))
        self._small, self._ints, self._digits, self._cand = {}, {}, {}, {}
        self.plan = list(plan)

    def small(self, b):
        if b not in self._small:
            ob = self.po.Oracle(self.oparams(1 << b, decomp_n=self.plan))
            self._small[b] = (ob, ob.keys_prepare(self.evk))
        return self._small[b]


def test_other_decompositions(po):
    """(4,4,4) at 9 bits is the plan [4,4,1]; (2,2,2,2,2,2) at 11 bits is six digits, more than a selector holds"""
    w = PlanWorld(po, (4, 4, 4), seed=430)
    b = 9
    assert po.get_base_2d(1 << b, [4, 4, 4]) == [[4, 4, 1]]
    bank = w.new_bank(2)
    bank._use_keys(w.keys)
    t, data, row = loaded_table(w, bank, b)
    idxs = [0, 511, 273]
    sels = [wide(w, bank, i, b) for i in idxs]
    assert sels[0].n_digits() == 3
    got = bank.table_read([t] * 3, sels)
    for k, (idx, want) in enumerate(zip(idxs, oracle_reads(w, b, row, idxs))):
        assert np.array_equal(got[k], want), (idx, np.count_nonzero(got[k] != want))
        decrypts_to(w, got[k], word_of(w, data, idx), False, ("(4,4,4)", idx))
    pkg = w.pkg
    assert po.get_base_2d(1 << 11, [2] * 6) == [[2, 2, 2, 2, 2, 1]]
    six = pkg.RamBank(pkg.Parameters(max_addr=1 << 12, word_size=2, decomp_n=[2] * 6), 1, 0)
    with pytest.raises(pkg.FheRamError) as e:
        six.table_selector(11)
    assert e.value.code == ST_UNSUPPORTED and "digits" in e.value.msg, e.value
    assert six.table_selector(10).n_digits() == 5


# ---- 7. the new source kind -------------------------------------------------------------------------------------------------------------------------
def test_table_result_as_candidate_lane_and_written_word(w2):
    w, pkg, S, L = w2, w2.pkg, w2.pkg.Src, w2.pkg.Lane
    assert (S.table(1).kind, L.table(1, 0).kind) == (8, 8)
    bank = w.new_bank(2)
    bank._use_keys(w.keys)
    vals, cts = w.candidates(1, seed=50)
    en = [narrow_selector(w, bank, e, 1) for e in (0, 1)]
    with pytest.raises(pkg.FheRamError) as e:
        bank.select([en[0]], [[S.table(0), S.zero()]])
    assert e.value.code == ST_STATE, "TABLE_RESULT before any table read"
    with pytest.raises(pkg.FheRamError) as e:
        bank.table_result(0, 1)
    assert e.value.code == ST_STATE
    t, data, row = loaded_table(w, bank, 9)
    tres = bank.table_read([t, t], [wide(w, bank, 100, 9), wide(w, bank, 401, 9)])
    # a select candidate
    for pick in (0, 1):
        got = bank.select([en[pick]], [[S.table(1), S.host(0)]], host_words=cts)[0]
        assert np.array_equal(got, w.oselect(1, np.stack([tres[1], cts[0]]), enc_digits(w, pick, 1))), pick
    decrypts_to(w, bank.select([en[0]], [[S.table(1), S.host(0)]], host_words=cts)[0], word_of(w, data, 401), False, "table word through a select")
    # a lane
    cands = [[L.table(0, 1), L.table(1, 0)], [L.zero(), L.table(0, 0)]]
    words = np.stack([np.stack([tres[0][1], tres[1][0]]), np.stack([np.zeros_like(tres[0][0]), tres[0][0]])])
    for pick in (0, 1):
        got = bank.select_lanes([en[pick]], [cands])[0]
        assert np.array_equal(got, w.oselect(1, words, enc_digits(w, pick, 1))), pick
    # a register write's word
    rb, rd = 3, 5
    rdata, rrow = regs_rows(w, rb)
    rf = bank.regfile(rb)
    rf.load(rrow)
    sel = narrow_selector(w, bank, rd, rb)
    rf.read_prepare_write(sel, download=False)
    rf.write(sel, S.table(0))
    oram, okeys = oram_of(w, rb, rrow), w.small(rb)[1]
    oram.read_prepare_write(oaddr(w, rd, rb), okeys)
    oram.write(tres[0], oaddr(w, rd, rb), okeys)
    assert np.array_equal(rf.store(), orow(w, oram))
    rf.pack([S.table(1), S.zero()])
    assert np.array_equal(rf.read([narrow_selector(w, bank, 0, rb)])[0], w.oselect(rb, np.stack([tres[1], np.zeros_like(tres[1])]), enc_digits(w, 0, rb)))
    # kind 7 stays unknown, an output outside the last table read too
    for bad in (S(7, 0), S.table(2)):
        with pytest.raises(pkg.FheRamError) as e:
            bank.select([en[0]], [[bad, S.zero()]])
        assert e.value.code == ST_INVALID_ARG, (bad.kind, e.value)


# ---- 8. isolation -------------------------------------------------------------------------------------------------------------------------------------
def test_a_table_read_inside_a_members_and_a_register_files_write(w2):
    """member 0 sits between read_prepare_write and write, and a register file between its own two halves, while a table is read"""
    w, S = w2, w2.pkg.Src
    rb = 5
    rdata, rrow = regs_rows(w, rb)
    vals, cts = w.candidates(3, seed=51)
    bank = w.new_bank(2)
    a = w.addrs
    lst = bank.read_list([1, 0], [a[1], a[2]], w.keys)
    picked = bank.select([narrow_selector(w, bank, 1, 1)], [[S.host(0), S.list(0)]], host_words=cts)
    rf = bank.regfile(rb)
    rf.load(rrow)
    rsel = narrow_selector(w, bank, 11, rb)
    regs = rf.read([rsel, narrow_selector(w, bank, 3, rb)])
    bank.read_prepare_write([a[0]], w.keys, first=0)
    rf.read_prepare_write(rsel, download=False)

    def digest():
        return (sha(bank.list_result(0, 2)), sha(bank.select_result(0, 1)), sha(rf.result(0, 2)), sha(rf.old_result()), sha(bank.result(0, 2)),
                sha(bank.store_encrypted(1)), sha(rf.store()), bank.state(0), bank.state(1), rf.state())

    before = digest()
    t, data, row = loaded_table(w, bank, 12)
    got = bank.table_read([t, t], [wide(w, bank, 9, 12), wide(w, bank, 4000, 12)], download=False)
    assert got is None
    got = bank.table_result(0, 2)
    for k, want in enumerate(oracle_reads(w, 12, row, [9, 4000])):
        assert np.array_equal(got[k], want), k
    assert digest() == before, "a table read moved something of the bank"
    assert np.array_equal(bank.list_result(0, 2), lst) and np.array_equal(bank.select_result(0, 1), picked) and np.array_equal(rf.result(0, 2), regs)
    # both writes resume exactly as the oracle's RAMs do
    rf.write(rsel, S.host(2), host_words=cts)
    oram, okeys = oram_of(w, rb, rrow), w.small(rb)[1]
    oram.read_prepare_write(oaddr(w, 11, rb), okeys)
    oram.write(cts[2], oaddr(w, 11, rb), okeys)
    assert np.array_equal(rf.store(), orow(w, oram)) and not rf.state()
    om = w.new_oram(0)
    om.read_prepare_write(w.o.address_new(w.addr_g[0]), w.okeys)
    om.write(cts[1], w.o.address_new(w.addr_g[0]), w.okeys)
    bank.write(cts[1:2], [a[0]], w.keys, first=0)
    assert np.array_equal(bank.store_encrypted(0), om.store()), np.count_nonzero(bank.store_encrypted(0) != om.store())
    assert not bank.state(0)
    assert sha(t.download()) == sha(row)


# ---- 9. refusals, lifetimes -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(w2):
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    L = lib()
    b = 9
    bank, other, fresh = w.new_bank(2), w.new_bank(1), w.new_bank(2)   # fresh: keys not loaded
    bank._use_keys(w.keys)
    other._use_keys(w.keys)
    t, data, row = loaded_table(w, bank, b)
    t_other, _, _ = loaded_table(w, other, b)
    t_fresh, _, _ = loaded_table(w, fresh, b)
    t_empty, t12 = bank.table(b), bank.table(12)
    t12.load(regs_rows(w, 12)[1])
    sel, sel12, empty = wide(w, bank, 77, b), wide(w, bank, 77, 12), bank.table_selector(b)
    foreign = wide(w, other, 77, b)
    rf = bank.regfile(5)
    rf.load(regs_rows(w, 5)[1])
    first = bank.table_read([t], [sel])[0]

    def digest():
        return sha(t.download()), sha(bank.table_result(0, 1)), [sha(bank.store_encrypted(m)) for m in range(2)], sha(rf.store()), rf.state()

    def refused(code, call, what):
        before = digest()
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg, what
        assert digest() == before, what

    # -- create
    refused(ST_INVALID_ARG, lambda: bank.table(0), "bits 0")
    refused(ST_INVALID_ARG, lambda: bank.table(13), "bits 13")
    refused(ST_INVALID_ARG, lambda: bank.table_selector(0), "a selector of 0 bits")
    refused(ST_INVALID_ARG, lambda: bank.table_selector(13), "a selector of 13 bits")
    refused(ST_INVALID_ARG, lambda: bank.table_selector_fields([7, 6]), "widths that sum to 13")
    refused(ST_INVALID_ARG, lambda: bank.table_selector_fields([2] * 6), "six fields")
    refused(ST_INVALID_ARG, lambda: bank.table_selector_fields([4, 0]), "a field of no bits")
    refused(ST_INVALID_ARG, lambda: bank.table_selector(b, list(enc_digits(w, 77, b))[:2]), "two digits for a plan of three")
    refused(ST_INVALID_ARG, lambda: bank.selector(6), "fheram_bank_selector_alloc keeps its bound")
    refused(ST_INVALID_ARG, lambda: bank.selector_fields([3, 3]), "fheram_bank_selector_alloc_fields keeps its bound")
    refused(ST_INVALID_ARG, lambda: pkg.Selector.from_digits(bank, 6, list(enc_digits(w, 5, 6))), "fheram_bank_selector_create keeps its bound")
    refused(ST_INVALID_ARG, lambda: bank.regfile(6), "a register file keeps its bound")
    out = C.c_void_p()
    assert L.fheram_bank_table_create(bank._h, b, None) == ST_INVALID_ARG and L.fheram_bank_table_create(None, b, C.byref(out)) == ST_INVALID_ARG
    assert L.fheram_bank_table_selector_alloc(bank._h, b, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_selector_create(bank._h, None, 3, b, C.byref(out)) == ST_INVALID_ARG
    assert L.fheram_bank_table_selector_alloc_fields(bank._h, None, 2, C.byref(out)) == ST_INVALID_ARG
    # -- read
    refused(ST_INVALID_ARG, lambda: bank.table_read([t], [sel12]), "a selector of other bits")
    refused(ST_INVALID_ARG, lambda: bank.table_read([t12], [sel]), "a table of other bits")
    refused(ST_INVALID_ARG, lambda: bank.table_read([t], [empty]), "an empty selector")
    refused(ST_INVALID_ARG, lambda: bank.table_read([t], [foreign]), "a selector of another bank")
    refused(ST_INVALID_ARG, lambda: bank.table_read([t_other], [sel]), "a table of another bank")
    refused(ST_INVALID_ARG, lambda: bank.table_read([t, t12], [sel, sel12]), "three digits beside four")
    refused(ST_INVALID_ARG, lambda: bank.table_read([t] * 9, [sel] * 9), "n = 9")
    refused(ST_UNINITIALIZED, lambda: bank.table_read([t, t_empty], [sel, sel]), "no upload or load yet")
    refused(ST_UNINITIALIZED, lambda: t_empty.download(), "download before any upload")
    refused(ST_KEYS, lambda: fresh.table_read([t_fresh], [wide(w, fresh, 77, b)]), "keys not loaded")
    refused(ST_INVALID_ARG, lambda: bank.table_result(1, 1), "result outside the last read")
    refused(ST_INVALID_ARG, lambda: bank.table_result(0, 0), "an empty result")
    pt, ps = (C.c_void_p * 1)(t._h), (C.c_void_p * 1)(sel._h)
    assert L.fheram_bank_table_read(None, pt, ps, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_read(bank._h, None, ps, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_read(bank._h, pt, None, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_read(bank._h, pt, ps, 0, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_read(bank._h, (C.c_void_p * 1)(None), ps, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_read(bank._h, pt, (C.c_void_p * 1)(None), 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_result(bank._h, 0, 1, None) == ST_INVALID_ARG and L.fheram_bank_table_result(None, 0, 1, None) == ST_INVALID_ARG
    # -- upload, download, load_plain
    refused(ST_RANGE, lambda: t.load(np.full_like(row, 1 << 17)), "an upload out of range")
    assert L.fheram_bank_table_upload(bank._h, t._h, None) == ST_INVALID_ARG and L.fheram_bank_table_download(bank._h, t._h, None) == ST_INVALID_ARG
    assert L.fheram_bank_table_upload(bank._h, t_other._h, row.ctypes.data_as(I64P)) == ST_INVALID_ARG
    assert L.fheram_bank_table_upload(None, t._h, row.ctypes.data_as(I64P)) == ST_INVALID_ARG
    plain = np.zeros((1 << b) * w.ws, dtype=np.uint8)
    pp = plain.ctypes.data_as(U8P)
    before = digest()
    assert L.fheram_bank_table_load_plain(bank._h, t._h, pp, plain.size - 1) == ST_INVALID_ARG, "a wrong data_len"
    assert L.fheram_bank_table_load_plain(bank._h, t._h, pp, plain.size * 2) == ST_INVALID_ARG
    assert L.fheram_bank_table_load_plain(bank._h, t._h, None, plain.size) == ST_INVALID_ARG
    assert L.fheram_bank_table_load_plain(bank._h, t_other._h, pp, plain.size) == ST_INVALID_ARG
    assert L.fheram_bank_table_load_plain(None, t._h, pp, plain.size) == ST_INVALID_ARG
    assert digest() == before
    assert L.fheram_table_bits(None) == 0
    # -- a wide selector is no select's and no register file's
    refused(ST_INVALID_ARG, lambda: bank.select([sel], [[S.zero(), S.zero()]]), "a wide selector in select")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([sel], [[[pkg.Lane.zero()] * w.ws]]), "a wide selector in select_lanes")
    refused(ST_INVALID_ARG, lambda: rf.read([sel]), "a wide selector in regs_read")
    # a narrow selector made by the wide call is an ordinary selector
    five = wide(w, bank, 19, 5)
    assert np.array_equal(rf.read([five])[0], rf.read([narrow_selector(w, bank, 19, 5)])[0])
    # a valid read behind the refusals
    assert np.array_equal(bank.table_read([t], [sel])[0], first)
    # lifetimes: a table destroyed before its bank; a bank destroyed first leaves handles that only fheram_table_destroy may take, and takes
    h = t12._h
    t12._h = None
    L.fheram_table_destroy(h)
    assert np.array_equal(bank.table_read([t], [sel])[0], first), "the bank and its other tables still work"
    hb, h2 = other._h, t_other._h
    other._h = None
    t_other._h = None
    L.fheram_bank_destroy(hb)
    assert L.fheram_table_bits(h2) == b
    L.fheram_table_destroy(h2)
    L.fheram_table_destroy(None)
    assert np.array_equal(bank.table_result(0, 1)[0], first)
