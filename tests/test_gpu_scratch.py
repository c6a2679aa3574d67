"""Wide register files (fheram_bank_regs_create_wide, fheram_bank_regs_peek / _poke; RamBank.scratch, RegFile.peek / poke): a
writable one-row memory of up to 4096 words beside the members of a bank, addressed by wide selectors.

The contract, in the oracle's own operations: with ob = Oracle(OParams(max_addr = 2^b, word_size = ws)) (SelWorld.small(b)) and its one-row
RAM, RegFile.read / read_prepare_write / write are ORam.read / read_prepare_write / write at address_new(selector digits) for every b up
to 12, and peek / poke are the members' (tests/test_gpu_public_io.py) on the one row.  Every comparison is np.array_equal on int64; the
noise of a decrypted output is printed, not bounded.  Banks are at max_addr = 2^12 (one row, one coordinate) with 2 members and
word_size = 2 unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import lib, sha
from test_gpu_regs import (bank2, decrypts_to, enc_digits, oaddr, oram_of, orow, regs_rows, w2, w13, word_of)  # noqa: F401 (w2, w13, bank2: fixtures)
from test_gpu_regs import selector as narrow_selector
from test_gpu_select import VALUE

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS = 1, 2, 3, 4
PLANS = {6: [3, 3], 9: [3, 3, 3], 12: [3, 3, 3, 3]}
FIVE = [3, 3, 2, 2, 2]
_CYCLES = {}


def wide(w, bank, idx, b):
    """the selector of index idx of a register file of b bits, from freshly encrypted host digits: wide above 5 bits"""
    return bank.table_selector(b, list(enc_digits(w, idx, b))) if b > 5 else narrow_selector(w, bank, idx, b)


def loaded(w, bank, b, seed=0):
    data, row = regs_rows(w, b, seed)
    rf = bank.scratch(b)
    rf.load(row)
    return rf, data, row


def oracle_cycle(w, b, row, idx, word, others, seed=0):
    """one write cycle of the oracle's one-row RAM, computed once: (old word, rotated row, row after the write, the reads at [idx] + others)"""
    key = (id(w), b, seed, idx, sha(word), tuple(others))
    if key not in _CYCLES:
        oram, okeys = oram_of(w, b, row), w.small(b)[1]
        old = oram.read_prepare_write(oaddr(w, idx, b), okeys)
        rotated = orow(w, oram).copy()
        oram.write(word, oaddr(w, idx, b), okeys)
        _CYCLES[key] = (old, rotated, orow(w, oram).copy(), [oram.read(oaddr(w, i, b), okeys) for i in [idx] + list(others)])
    return _CYCLES[key]


def five_world(w, bank):
    """(oracle of DECOMP_N = [3,3,2,2,2] at 2^12, its keys, a (3,3,2,2,2) field selector of the bank at index = bits [0, 12) of VALUE, the
    selector's digits, the index)"""
    ob = w.po.Oracle(w.oparams(1 << 12, decomp_n=FIVE))
    assert w.po.get_base_2d(1 << 12, FIVE) == [FIVE]
    fu = w.pkg.FheUintPrepared.from_host(bank, w.bits(VALUE))
    f = bank.table_selector_fields(FIVE)
    assert f.n_digits() == 5 and f.bits == 12
    bank.derive_selector_fields(f, [fu] * 5, [0, 3, 6, 8, 10])
    digits = ob.address_from_fheuint(w.bits(VALUE)[0:12], sign=False)
    assert np.array_equal(f.download(), digits)
    return ob, ob.keys_prepare(w.evk), f, digits, VALUE & 4095


# ---- 1. read -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [6, 9, 12])
def test_read_equals_the_oracle(w2, bank2, b):
    """two, three and four digits; index 0, 2^b - 1 and a middle one in ONE call, one selector twice; the row does not change"""
    w = w2
    assert w.small(b)[0].n_digits == len(PLANS[b])
    rf, data, row = loaded(w, bank2, b)
    assert rf.bits == b and lib().fheram_regs_bits(rf._h) == b and not rf.state()
    assert np.array_equal(rf.store(), row)
    idxs = [0, (1 << b) - 1, (1 << b) // 2 + 5]
    sels = [wide(w, bank2, i, b) for i in idxs]
    assert all(s.n_digits() == len(PLANS[b]) for s in sels)
    sels.append(sels[1])
    idxs.append(idxs[1])
    got = rf.read(sels)
    assert got.shape == (4, w.ws, w.params.glwe_len())
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    for k, idx in enumerate(idxs):
        want = oram.read(oaddr(w, idx, b), okeys)
        assert np.array_equal(got[k], want), (b, k, idx, np.count_nonzero(got[k] != want))
        noise = decrypts_to(w, got[k], word_of(w, data, idx), False, (b, idx))
        print(f"scratch read b={b} idx={idx}: log2 noise {noise:.2f}")
    assert sha(rf.store()) == sha(row) and not rf.state(), "a read changed the register file"
    assert rf.read(sels[:2], download=False) is None
    assert np.array_equal(rf.result(0, 2), got[:2]) and np.array_equal(rf.result(1, 1)[0], got[1])


# ---- 2. read_prepare_write / write ---------------------------------------------------------------------------------------------------------------
CONFIGS = [None, {"memo": 0}, {"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}]


@pytest.mark.parametrize("config", CONFIGS, ids=["default", "memo0", "safe_monitor2", "tail0_fuse0"])
@pytest.mark.parametrize("b", [6, 9, 12])
def test_write_cycle_equals_the_oracle(w2, b, config):
    w, S = w2, w2.pkg.Src
    idx, others = (1 << b) // 3, [0, (1 << b) - 1]
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=60)
    bank = w.new_bank(2, config=config)
    bank._use_keys(w.keys)
    rf = bank.scratch(b)
    rf.load(row)
    want_old, want_rotated, want_row, want_reads = oracle_cycle(w, b, row, idx, cts[0], others)
    sel = wide(w, bank, idx, b)
    old = rf.read_prepare_write(sel)
    assert np.array_equal(old, want_old), np.count_nonzero(old != want_old)
    assert np.array_equal(rf.old_result(), old)
    assert np.array_equal(rf.store(), want_rotated), "the rotated row"
    assert rf.state()
    decrypts_to(w, old, word_of(w, data, idx), False, "the old word")
    rf.write(sel, S.host(0), host_words=cts)
    assert np.array_equal(rf.store(), want_row), "the row after the write"
    assert not rf.state()
    got = rf.read([sel] + [wide(w, bank, i, b) for i in others])
    for k, i in enumerate([idx] + others):
        assert np.array_equal(got[k], want_reads[k]), (i, np.count_nonzero(got[k] != want_reads[k]))
    noise = decrypts_to(w, got[0], vals[0], True, "the written word")
    for k, i in enumerate(others):
        noise = max(noise, decrypts_to(w, got[1 + k], word_of(w, data, i), False, ("untouched word", i)))
    print(f"scratch write cycle b={b} {config}: log2 noise {noise:.2f}, round-off maximum {bank.roundoff_max():.4f}")
    assert sha(bank.store_encrypted(0)) == sha(w.rows[0]) and sha(bank.store_encrypted(1)) == sha(w.rows[1])


def test_three_write_cycles(w2, bank2):
    w, S = w2, w2.pkg.Src
    b = 12
    data, row = regs_rows(w, b, seed=1)
    vals, cts = w.candidates(3, seed=61)
    rf = bank2.scratch(b)
    rf.load(row)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    for k, idx in enumerate([0, 4095, 1365]):
        sel = wide(w, bank2, idx, b)
        assert rf.read_prepare_write(sel, download=False) is None
        oram.read_prepare_write(oaddr(w, idx, b), okeys)
        rf.write(sel, S.host(k), host_words=cts)
        oram.write(cts[k], oaddr(w, idx, b), okeys)
        assert np.array_equal(rf.store(), orow(w, oram)), ("cycle", k)
        assert not rf.state()
    got = rf.read([wide(w, bank2, i, b) for i in (0, 4095, 1365, 7)])
    noise = max([decrypts_to(w, got[k], vals[k], True) for k in range(3)] + [decrypts_to(w, got[3], word_of(w, data, 7), False, "never written")])
    print(f"scratch three cycles: log2 noise {noise:.2f}")


# ---- 3. five digits -------------------------------------------------------------------------------------------------------------------------------
def test_five_digit_field_selector(w2, bank2):
    """widths (3,3,2,2,2): the Address of an oracle whose DECOMP_N is [3,3,2,2,2]; five products are more than the tail launch takes"""
    w, S = w2, w2.pkg.Src
    ob, okeys, f, digits, index = five_world(w, bank2)
    rf, data, row = loaded(w, bank2, 12)
    vals, cts = w.candidates(1, seed=62)
    oram = ob.ram_new()
    oram.load(row.reshape(w.ws, 1, -1))
    addr = ob.address_new(digits)
    got = rf.read([f])[0]
    assert np.array_equal(got, oram.read(addr, okeys))
    decrypts_to(w, got, word_of(w, data, index), False, "the word at the five fields")
    old = rf.read_prepare_write(f)
    assert np.array_equal(old, oram.read_prepare_write(addr, okeys)) and np.array_equal(old, got)
    assert np.array_equal(rf.store(), orow(w, oram)) and rf.state()
    rf.write(f, S.host(0), host_words=cts)
    oram.write(cts[0], addr, okeys)
    assert np.array_equal(rf.store(), orow(w, oram)) and not rf.state()
    back = rf.read([f])[0]
    assert np.array_equal(back, oram.read(addr, okeys))
    noise = decrypts_to(w, back, vals[0], True, "the written word")
    print(f"scratch (3,3,2,2,2) cycle at index {index}: log2 noise {noise:.2f}")


# ---- 4. the member path and the one-row path are one reference operation ----------------------------------------------------------------------
def test_twin_member(w2):
    w, pkg = w2, w2.pkg
    b, idx = 12, 2741
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=63)
    bank = w.new_bank(2)
    bank._use_keys(w.keys)
    bank.load_encrypted(0, row.reshape(w.ws, 1, -1))
    rf = bank.scratch(b)
    rf.load(row)
    digits = list(enc_digits(w, idx, b))
    addr, sel = pkg.Address(w.params, digits), bank.table_selector(b, digits)

    def same(what):
        m, r = bank.store_encrypted(0).reshape(w.ws, -1), rf.store()
        assert np.array_equal(m, r), (what, np.count_nonzero(m != r))

    assert np.array_equal(bank.read([addr], w.keys, first=0)[0], rf.read([sel])[0])
    same("read")
    assert np.array_equal(bank.read_prepare_write([addr], w.keys, first=0)[0], rf.read_prepare_write(sel))
    same("read_prepare_write")
    bank.write(cts[0:1], [addr], w.keys, first=0)
    rf.write(sel, pkg.Src.host(0), host_words=cts)
    same("write")
    assert not bank.state(0) and not rf.state()


# ---- 5. every word source of a write ----------------------------------------------------------------------------------------------------------------
def test_every_word_source_of_a_write(w2):
    w, S = w2, w2.pkg.Src
    b = 9
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(2, seed=64)
    bank = w.new_bank(2)
    bank.read([w.addrs[0]], w.keys, first=0)
    bank.select([narrow_selector(w, bank, 1, 1)], [[S.host(0), S.host(1)]], host_words=cts, download=False)
    t = bank.table(b)
    t.load(regs_rows(w, b, seed=1)[1])
    bank.table_read([t], [wide(w, bank, 77, b)], download=False)
    bank.peek([1], [33], download=False)
    rf = bank.scratch(b)
    rf.load(row)
    rf.read([wide(w, bank, 2, b), wide(w, bank, 500, b)], download=False)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    zero = np.zeros((w.ws, w.params.glwe_len()), dtype=np.int64)
    sources = [("ZERO", S.zero(), None, lambda: zero), ("HOST", S.host(1), cts, lambda: cts[1]), ("MEMBER_RESULT", S.member(0), None, lambda: bank.result(0, 1)[0]),
               ("SELECT_RESULT", S.select(0), None, lambda: bank.select_result(0, 1)[0]), ("REGS_RESULT", S.regs(1), None, lambda: rf.result(1, 1)[0]),
               ("REGS_OLD", S.regs_old(), None, lambda: rf.old_result()), ("TABLE_RESULT", S.table(0), None, lambda: bank.table_result(0, 1)[0]),
               ("PEEK_RESULT", S.peek(0), None, lambda: bank.peek_result(0, 1)[0])]
    for k, (name, src, hw, fetch) in enumerate(sources):
        idx = (67 * k + 1) % (1 << b)
        sel = wide(w, bank, idx, b)
        rf.read_prepare_write(sel, download=False)
        oram.read_prepare_write(oaddr(w, idx, b), okeys)
        rf.write(sel, src, host_words=hw)
        oram.write(fetch(), oaddr(w, idx, b), okeys)
        assert np.array_equal(rf.store(), orow(w, oram)), name
        assert not rf.state(), name
    w.check_value(rf.read([wide(w, bank, 1, b)])[0], None, "the word ZERO was written to")


# ---- 6. the write enable ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enable", [0, 1])
def test_write_enable_without_a_sync(w2, bank2, enable):
    """word <- enable ? new : old, all on the device: the select is over [REGS_OLD, HOST] by a NARROW 1-bit selector, the write goes to the wide file"""
    w, S = w2, w2.pkg.Src
    b, rd = 12, 3000
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=65)
    rf = bank2.scratch(b)
    rf.load(row)
    sel, en = wide(w, bank2, rd, b), narrow_selector(w, bank2, enable, 1)
    rf.read_prepare_write(sel, download=False)
    bank2.select([en], [[S.regs_old(), S.host(0)]], host_words=cts, download=False)
    rf.write(sel, S.select(0))
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    old = oram.read_prepare_write(oaddr(w, rd, b), okeys)
    picked = w.oselect(1, np.stack([old, cts[0]]), enc_digits(w, enable, 1))
    oram.write(picked, oaddr(w, rd, b), okeys)
    assert np.array_equal(rf.old_result(), old)
    assert np.array_equal(bank2.select_result(0, 1)[0], picked)
    assert np.array_equal(rf.store(), orow(w, oram)) and not rf.state()
    got = rf.read([sel, wide(w, bank2, 0, b)])
    noise = decrypts_to(w, got[0], vals[0] if enable else word_of(w, data, rd), bool(enable), "the word behind the enable")
    noise = max(noise, decrypts_to(w, got[1], word_of(w, data, 0), False, "untouched"))
    print(f"scratch write enable = {enable}: log2 noise {noise:.2f}")


# ---- 7. selectors out of one derive list ------------------------------------------------------------------------------------------------------------
def test_index_and_rd_from_one_derive_list(w2, bank2):
    """the index = bits [2, 14) of an encrypted integer and a 5-bit rd = bits [7, 12) in ONE launch; then a cycle on a 12-bit and on a 5-bit file"""
    w, pkg, S, D = w2, w2.pkg, w2.pkg.Src, w2.pkg.Derive
    vals, cts = w.candidates(2, seed=66)
    fu = pkg.FheUintPrepared.from_host(bank2, w.bits(VALUE))
    at, rd = bank2.table_selector(12), bank2.selector(5)
    bank2.profile_enable(True)
    bank2.profile_reset()
    bank2.derive_list([D.selector(fu, at, 2), D.selector(fu, rd, 7)])
    bank2.sync()
    prof = bank2.profile_get("derive")
    bank2.profile_enable(False)
    assert prof["launches"] == 1 and prof["blocks"] == 6 * (4 + 2), prof
    noise = -1e9
    for k, (b, sel, f) in enumerate([(12, at, 2), (5, rd, 7)]):
        data, row = regs_rows(w, b)
        rf = bank2.scratch(b)
        rf.load(row)
        ob, okeys = w.small(b)
        oram, a = oram_of(w, b, row), ob.address_new(w.digits(VALUE, f, b))
        assert np.array_equal(sel.download(), w.digits(VALUE, f, b))
        rf.read_prepare_write(sel, download=False)
        rf.write(sel, S.host(k), host_words=cts)
        assert np.array_equal(rf.old_result(), oram.read_prepare_write(a, okeys))
        oram.write(cts[k], a, okeys)
        assert np.array_equal(rf.store(), orow(w, oram)), b
        noise = max(noise, decrypts_to(w, rf.read([sel])[0], vals[k], True, ("derived", b)))
    print(f"scratch cycles at derived selectors (index {(VALUE >> 2) & 4095}, rd {(VALUE >> 7) & 31}): log2 noise {noise:.2f}")


# ---- 8. mixed operations ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bits12", "five_digits"])
def test_mixed_operations(w2, form):
    """the wide file as the regs / prepare_regs group of read_mix and read_prepare_write_mix: each output equals the single call's, and the
    write behind them gives the oracle's row.  bits12: four digits (the mix's one-launch top); five_digits: the groups run entry by entry"""
    w, S = w2, w2.pkg.Src
    b = 12
    bank = w.new_bank(2)
    bank._use_keys(w.keys)
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=67)
    if form == "bits12":
        ob, okeys = w.small(b)
        sels = [wide(w, bank, 4095, b), wide(w, bank, 1234, b)]
        addr = oaddr(w, 1234, b)
    else:
        ob, okeys, f, digits, index = five_world(w, bank)
        sels = [f, f]
        addr = ob.address_new(digits)
    rf, ref = bank.scratch(b), bank.scratch(b)
    rf.load(row)
    ref.load(row)
    a = w.addrs
    single = ref.read(sels)
    single_list = bank.read_list([1], [a[1]], w.keys)
    lst, tab, regs = bank.read_mix(list=([1], [a[1]]), regs=(rf, sels))
    assert tab is None and np.array_equal(regs, single) and np.array_equal(lst, single_list)
    assert np.array_equal(rf.result(0, 2), single)
    single_old = ref.read_prepare_write(sels[1])
    lst, tab, regs, plist, pregs = bank.read_prepare_write_mix(regs=(rf, sels[:1]), prepare_regs=(rf, sels[1]))
    assert lst is None and tab is None and plist is None
    assert np.array_equal(regs[0], single[0]) and np.array_equal(pregs, single_old)
    assert rf.state() and np.array_equal(rf.store(), ref.store()) and np.array_equal(rf.old_result(), single_old)
    rf.write(sels[1], S.host(0), host_words=cts)
    oram = ob.ram_new()
    oram.load(row.reshape(w.ws, 1, -1))
    assert np.array_equal(single_old, oram.read_prepare_write(addr, okeys))
    oram.write(cts[0], addr, okeys)
    assert np.array_equal(rf.store(), orow(w, oram)) and not rf.state()
    noise = decrypts_to(w, rf.read(sels[1:])[0], vals[0], True, form)
    print(f"scratch mixed operations {form}: log2 noise {noise:.2f}")


# ---- 9. peek / poke -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [5, 12])
def test_peek_and_poke_equal_the_twin_members(w2, b):
    """member 0 of the bank holds the register file's row: a public index i of the one row is address i of that member"""
    w, S = w2, w2.pkg.Src
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(3, seed=68)
    bank = w.new_bank(2)
    bank._use_keys(w.keys)
    bank.load_encrypted(0, row.reshape(w.ws, 1, -1))
    rf = bank.scratch(b)
    rf.load(row)
    top = (1 << b) - 1
    idxs = [0, top, top // 3, top // 2 + 1]
    before = (sha(rf.store()), rf.state(), sha(bank.store_encrypted(0)), sha(bank.store_encrypted(1)))
    want = bank.peek([0] * 4, idxs)
    got = rf.peek(idxs)
    assert np.array_equal(got, want), np.count_nonzero(got != want)
    assert np.array_equal(bank.peek_result(0, 4), got)
    assert rf.peek(idxs[:2], download=False) is None and np.array_equal(bank.peek_result(0, 2), got[:2])
    assert (sha(rf.store()), rf.state(), sha(bank.store_encrypted(0)), sha(bank.store_encrypted(1))) == before, "a peek changed something"
    for k, i in enumerate(idxs):
        noise = decrypts_to(w, got[k], word_of(w, data, i), False, ("peek", b, i))
        print(f"scratch peek b={b} idx={i}: log2 noise {noise:.2f}")
    # a poke of three distinct indices from HOST and ZERO sources
    targets, srcs = [top, 0, top // 3], [S.host(1), S.zero(), S.host(0)]
    bank.poke([0] * 3, targets, words=cts, srcs=srcs)
    want_old, want_row = bank.peek_result(0, 3), bank.store_encrypted(0).reshape(w.ws, -1)
    rf.poke(targets, words=cts, srcs=srcs)
    assert np.array_equal(bank.peek_result(0, 3), want_old), "the old words"
    assert np.array_equal(rf.store(), want_row), np.count_nonzero(rf.store() != want_row)
    assert not rf.state() and sha(bank.store_encrypted(1)) == before[3]
    # a read at an encrypted selector returns the poked word; the kept trace is void: a cycle behind the poke gives the oracle's row
    sel = wide(w, bank, top, b)
    oram, okeys = oram_of(w, b, want_row), w.small(b)[1]
    back = rf.read([sel, wide(w, bank, 0, b)])
    assert np.array_equal(back[0], oram.read(oaddr(w, top, b), okeys))
    noise = decrypts_to(w, back[0], vals[1], True, "the poked word")
    w.check_value(back[1], None, "the word ZERO was poked to")
    rf.read_prepare_write(sel, download=False)
    rf.write(sel, S.host(2), host_words=cts)
    oram.read_prepare_write(oaddr(w, top, b), okeys)
    oram.write(cts[2], oaddr(w, top, b), okeys)
    assert np.array_equal(rf.store(), orow(w, oram))
    # a poke between two cycles, its word taken from the peek before it
    rf.peek([top], download=False)
    rf.poke([1], srcs=[S.peek(0)])
    o2 = oram_of(w, b, rf.store())
    i2 = top // 3
    s2 = wide(w, bank, i2, b)
    rf.read_prepare_write(s2, download=False)
    rf.write(s2, S.zero())
    o2.read_prepare_write(oaddr(w, i2, b), okeys)
    o2.write(np.zeros_like(cts[0]), oaddr(w, i2, b), okeys)
    assert np.array_equal(rf.store(), orow(w, o2)), "a cycle behind a poke"
    noise = max(noise, decrypts_to(w, rf.read([wide(w, bank, 1, b)])[0], vals[2], True, "the peeked word poked to index 1"))
    print(f"scratch poke b={b}: log2 noise {noise:.2f}")


# ---- 10. the setup side ------------------------------------------------------------------------------------------------------------------------------
def test_setup_side_at_4096_words(w2, bank2):
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    b = 12
    ob, okeys = w.small(b)
    p = w.params
    dsk = pkg.GLWESecret(bank2, w.sk)
    data = np.random.default_rng(9100).integers(0, 256, size=(1 << b) * w.ws, dtype=np.uint8)
    rf = bank2.scratch(b)
    rf.load_plain(data)
    row = rf.store()
    assert not rf.state() and not np.any(row.reshape(w.ws, -1, 2, p.n())[:, :, 1, :]), "a mask limb is not zero"
    idxs = [0, 4095, 1365]
    got = rf.read([wide(w, bank2, i, b) for i in idxs])
    oram = oram_of(w, b, row)
    for k, i in enumerate(idxs):
        assert np.array_equal(got[k], oram.read(oaddr(w, i, b), okeys)), i
        decrypts_to(w, got[k], word_of(w, data, i), False, ("plain", i))
    rf.encrypt_sk(data, dsk, ob.source(9110), ob.source(9120))
    row = ob.ram_encrypt(data, w.sk, 9110, 9120).reshape(w.ws, -1)
    assert np.array_equal(rf.store(), row)
    vals, cts = w.candidates(2, seed=69)
    want = np.array([ob.expected_plain(int(x), ob.p.k_glwe_pt) for x in data]).reshape(-1, w.ws)
    for k, i in enumerate([4095, 2]):
        sel = wide(w, bank2, i, b)
        rf.read_prepare_write(sel, download=False)
        rf.write(sel, S.host(k), host_words=cts)
        want[i] = [ob.expected_plain(int(v), ob.p.k_glwe_pt, True) for v in vals[k]]
    values, worst = rf.decrypt(dsk)
    assert values.shape == (1 << b, w.ws) and np.array_equal(values, want), np.count_nonzero(values != want)
    print(f"scratch decrypt of 4096 words after two writes: worst log2 noise {worst:.2f}")


# ---- 11. isolation -------------------------------------------------------------------------------------------------------------------------------------
def test_a_wide_cycle_inside_a_members_write(w13):
    """at 2^13 (two rows, two coordinates): member 0 sits between read_prepare_write and write while a wide file is read, prepared and written"""
    w, S = w13, w13.pkg.Src
    b, idx = 12, 2222
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(3, seed=70)
    bank = w.new_bank(2)
    a = w.addrs
    lst = bank.read_list([1, 0], [a[1], a[2]], w.keys)
    picked = bank.select([narrow_selector(w, bank, 1, 1)], [[S.host(0), S.list(0)]], host_words=cts)
    t = bank.table(9)
    t.load(regs_rows(w, 9)[1])
    tab = bank.table_read([t], [wide(w, bank, 300, 9)])
    bank.read_prepare_write([a[0]], w.keys, first=0)

    def digest():
        return (sha(bank.list_result(0, 2)), sha(bank.select_result(0, 1)), sha(bank.table_result(0, 1)), sha(bank.result(0, 2)), sha(bank.tree(0, 0)),
                sha(bank.store_encrypted(1)), sha(t.download()))

    before = digest()
    rf = bank.scratch(b)
    rf.load(row)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    sel = wide(w, bank, idx, b)
    rf.read([sel, wide(w, bank, 3, b)], download=False)
    rf.read_prepare_write(sel, download=False)
    rf.write(sel, S.host(2), host_words=cts)
    oram.read_prepare_write(oaddr(w, idx, b), okeys)
    oram.write(cts[2], oaddr(w, idx, b), okeys)
    assert np.array_equal(rf.store(), orow(w, oram))
    assert [bank.state(0), bank.state(1)] == [True, False]
    assert digest() == before, "a wide register operation moved something of the bank"
    assert np.array_equal(bank.list_result(0, 2), lst) and np.array_equal(bank.select_result(0, 1), picked) and np.array_equal(bank.table_result(0, 1), tab)
    # the member resumes its write exactly as the oracle's RAM does
    om = w.new_oram(0)
    om.read_prepare_write(w.o.address_new(w.addr_g[0]), w.okeys)
    om.write(cts[1], w.o.address_new(w.addr_g[0]), w.okeys)
    bank.write(cts[1:2], [a[0]], w.keys, first=0)
    assert np.array_equal(bank.store_encrypted(0), om.store()), np.count_nonzero(bank.store_encrypted(0) != om.store())
    assert not bank.state(0)


# ---- 12. refusals, lifetimes ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(w2):
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    L = lib()
    bank, other = w.new_bank(2), w.new_bank(1)
    bank._use_keys(w.keys)
    other._use_keys(w.keys)
    vals, cts = w.candidates(1, seed=71)
    rf12, d12, r12 = loaded(w, bank, 12)
    rf5, d5, r5 = loaded(w, bank, 5)
    rf_empty = bank.scratch(9)
    s12, s9, s5 = wide(w, bank, 2741, 12), wide(w, bank, 300, 9), narrow_selector(w, bank, 19, 5)
    en = narrow_selector(w, bank, 1, 1)
    got12, got5 = rf12.read([s12]), rf5.read([s5], download=False)
    bank.select([en], [[S.host(0), S.zero()]], host_words=cts, download=False)
    rf12.peek([1], download=False)

    def digest():
        return (sha(rf12.store()), rf12.state(), sha(rf5.store()), rf5.state(), sha(rf12.result(0, 1)), sha(bank.select_result(0, 1)), sha(bank.peek_result(0, 1)),
                [sha(bank.store_encrypted(m)) for m in range(2)], [bank.state(m) for m in range(2)])

    def refused(code, call, what, say=None):
        before = digest()
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg and (say is None or say in e.value.msg), (what, e.value.msg)
        assert digest() == before, what

    def refused_by_the_library(call, what, say):
        """the C call itself, behind the Python mirror's own refusals"""
        before = digest()
        assert call() == ST_INVALID_ARG, what
        assert say in L.fheram_bank_last_error(bank._h).decode(), (what, L.fheram_bank_last_error(bank._h))
        assert digest() == before, what

    # -- selectors
    refused(ST_INVALID_ARG, lambda: rf12.read([s9]), "a selector of other bits", "bits")
    refused(ST_INVALID_ARG, lambda: rf5.read([s12]), "a 12-bit selector on a 5-bit file", "bits")
    refused(ST_INVALID_ARG, lambda: rf12.read([s5]), "a 5-bit selector on a 12-bit file", "bits")
    refused(ST_INVALID_ARG, lambda: rf12.read_prepare_write(s9), "read_prepare_write at a selector of other bits", "bits")
    refused(ST_INVALID_ARG, lambda: bank.select([s12], [[S.zero()]]), "a wide selector in select", "FHERAM_SELECT_BITS_MAX")
    # -- pack
    refused(ST_INVALID_ARG, lambda: rf12.pack([S.zero()] * 33), "pack of 33 candidates", "33 candidates")
    rf_pack = bank.scratch(12)
    rf_pack.pack([S.host(0)] + [S.zero()] * 31, host_words=cts)
    assert np.array_equal(rf_pack.read([wide(w, bank, 0, 12)])[0], w.oselect(12, np.stack([cts[0]]), enc_digits(w, 0, 12))), "a pack of 32 fills a wide file"
    rf12.read([s12], download=False)   # (the last register read is rf12's again)
    # -- creators
    u32, out = (C.c_uint32 * 2)(7, 7), C.c_void_p(1)
    src2 = (pkg.api._CSelectSrc * 2)(pkg.api._CSelectSrc(0, 0), pkg.api._CSelectSrc(0, 0))
    refused_by_the_library(lambda: L.fheram_bank_regs_create_wide(bank._h, 13, C.byref(out)), "regs_create_wide(13)", "FHERAM_TABLE_BITS_MAX = 12")
    assert out.value is None
    refused_by_the_library(lambda: L.fheram_bank_regs_create_wide(bank._h, 0, C.byref(out)), "regs_create_wide(0)", "FHERAM_TABLE_BITS_MAX = 12")
    assert L.fheram_bank_regs_create_wide(bank._h, 12, None) == ST_INVALID_ARG
    refused(ST_INVALID_ARG, lambda: bank.scratch(13), "scratch(13)")
    refused(ST_INVALID_ARG, lambda: bank.regfile(6), "regfile(6) is still refused", "FHERAM_SELECT_BITS_MAX = 5")
    # -- peek / poke
    refused(ST_UNINITIALIZED, lambda: rf_empty.peek([0]), "a peek on an uninitialised file")
    refused(ST_UNINITIALIZED, lambda: rf_empty.poke([0], srcs=[S.zero()]), "a poke on an uninitialised file")
    u32[0], u32[1] = 4096, 0
    refused_by_the_library(lambda: L.fheram_bank_regs_peek(bank._h, rf12._h, u32, 1, None), "a peek at index 2^bits", "outside the register file's 2^bits = 4096 words")
    refused_by_the_library(lambda: L.fheram_bank_regs_poke(bank._h, rf12._h, u32, 1, src2, None), "a poke at index 2^bits", "outside the register file's 2^bits = 4096 words")
    u32[0] = 32
    refused_by_the_library(lambda: L.fheram_bank_regs_peek(bank._h, rf5._h, u32, 1, None), "a peek at index 32 of a 5-bit file", "2^bits = 32 words")
    u32[0], u32[1] = 7, 7
    refused_by_the_library(lambda: L.fheram_bank_regs_poke(bank._h, rf12._h, u32, 2, src2, None), "a repeated poke target", "a second time")
    refused_by_the_library(lambda: L.fheram_bank_regs_peek(bank._h, rf12._h, u32, 17, None), "n = 17", "FHERAM_PEEK_MAX = 16")
    refused_by_the_library(lambda: L.fheram_bank_regs_peek(bank._h, rf12._h, None, 1, None), "a null index list", "null index list")
    refused_by_the_library(lambda: L.fheram_bank_regs_poke(bank._h, rf12._h, u32, 1, None, None), "null sources", "null")
    rf_other = other.scratch(12)
    refused_by_the_library(lambda: L.fheram_bank_regs_peek(bank._h, rf_other._h, u32, 1, None), "a register file of another bank", "another bank")
    refused(ST_INVALID_ARG, lambda: rf12.poke([7], srcs=[S(7, 0)]), "kind 7 in a poke")
    refused(ST_INVALID_ARG, lambda: rf12.poke([7], srcs=[S(9, 0)]), "kind 9 in a poke")
    refused(ST_INVALID_ARG, lambda: rf12.poke([7], srcs=[S.host(0)]), "HOST without words")
    rf12.read_prepare_write(s12, download=False)
    refused(ST_STATE, lambda: rf12.peek([0]), "a peek in state 1", "rotated")
    refused(ST_STATE, lambda: rf12.poke([0], srcs=[S.zero()]), "a poke in state 1", "rotated")
    rf12.write(s12, S.regs_old())
    assert not rf12.state()
    fresh = w.new_bank(2)   # keys not loaded
    rf_fresh = fresh.scratch(12)
    rf_fresh.load(r12)
    with pytest.raises(pkg.FheRamError) as e:
        rf_fresh.peek([0])
    assert e.value.code == ST_KEYS
    # -- both destroy orders
    h = rf5._h
    rf5._h = None
    L.fheram_regs_destroy(h)
    assert np.array_equal(rf_pack.read([wide(w, bank, 0, 12)], download=True)[0], w.oselect(12, np.stack([cts[0]]), enc_digits(w, 0, 12))), "the bank and its other files still work"
    hb, h2 = other._h, rf_other._h
    other._h = None
    rf_other._h = None
    L.fheram_bank_destroy(hb)
    assert L.fheram_regs_bits(h2) == 12
    L.fheram_regs_destroy(h2)
    assert np.array_equal(got12[0], oram_of(w, 12, r12).read(oaddr(w, 2741, 12), w.small(12)[1]))
    assert got5 is None
