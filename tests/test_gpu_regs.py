"""fheram_bank_regs_* (RamBank.regfile, RegFile): a bank's register file — a one-row RAM of 2^bits words that lives beside the members, is
read and written by the bank's selectors, feeds the selects and takes a written word from any source kind (include/fheram.h).

The contract, in the oracle's own operations: with ob = Oracle(OParams(max_addr = 2^b, word_size = ws)) (SelWorld.small(b)) and its one-row
RAM, RegFile.read / read_prepare_write / write are ORam.read / read_prepare_write / write at address_new(selector digits), and RegFile.pack is
the pack of RamBank.select.  Every comparison is np.array_equal on int64; the noise of a decrypted output is printed, not bounded (DESIGN.md
14, 17).  Banks are at max_addr = 2^12 (one row, one coordinate) with 2 members and word_size = 2 unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import lib, sha
from test_gpu_lanes import LaneWorld
from test_gpu_select import VALUE, SelWorld

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS, ST_RANGE = 1, 2, 3, 4, 6
I64P = C.POINTER(C.c_int64)
_ROWS, _DIGITS = {}, {}


def regs_rows(w, b, seed=0):
    """(bytes [2^b * ws], the encrypted one-row RAM [ws][GLWE]) of the oracle of max_addr = 2^b"""
    key = (id(w), b, seed)
    if key not in _ROWS:
        ob = w.small(b)[0]
        data = np.random.default_rng(7000 + 16 * seed + b).integers(0, 256, size=(1 << b) * w.ws, dtype=np.uint8)
        _ROWS[key] = (data, ob.ram_encrypt(data, w.sk, 7100 + 16 * seed + b, 7200 + 16 * seed + b).reshape(w.ws, -1))
    return _ROWS[key]


def enc_digits(w, idx, b):
    """the Address of index idx of that RAM, freshly encrypted: [n_digits][ggsw_len]"""
    key = (id(w), idx, b)
    if key not in _DIGITS:
        _DIGITS[key] = w.small(b)[0].address_encrypt(idx, w.sk, 7300 + 64 * b + idx, 7900 + 64 * b + idx)
    return _DIGITS[key]


def selector(w, bank, idx, b):
    return w.pkg.Selector.from_digits(bank, b, list(enc_digits(w, idx, b)))


def oaddr(w, idx, b):
    return w.small(b)[0].address_new(enc_digits(w, idx, b))


def oram_of(w, b, row):
    oram = w.small(b)[0].ram_new()
    oram.load(np.asarray(row).reshape(w.ws, 1, -1))
    return oram


def orow(w, oram):
    return oram.store().reshape(w.ws, -1)


def word_of(w, data, idx):
    return [int(data[i + w.ws * idx]) for i in range(w.ws)]


def decrypts_to(w, cts, values, written, what=""):
    """cts [ws][GLWE] decrypt to the bytes `values`; returns the largest log2 noise"""
    worst = -1e9
    for i in range(w.ws):
        want = w.o.expected_plain(int(values[i]), w.o.p.k_glwe_pt, written)
        v, noise = w.o.glwe_decrypt(cts[i], want, w.sk)
        assert v == want, (what, i, v, want, noise)
        worst = max(worst, noise)
    return worst


@pytest.fixture(scope="module")
def w2(po):
    return SelWorld(po, 1 << 12, 2, 2, seed=400)


@pytest.fixture(scope="module")
def w13(po):
    return SelWorld(po, 1 << 13, 2, 2, seed=410)


@pytest.fixture(scope="module")
def bank2(w2):
    """one default bank of two members shared by the tests that change no member's rows"""
    bank = w2.new_bank(2)
    bank._use_keys(w2.keys)
    return bank


# ---- 1. read ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 5])
def test_read_equals_the_oracle(w2, bank2, b):
    """the digit plans [1], [3] and [3, 2] (two digits: the products inside the tail launch); index 0, 2^b - 1 and a middle one in ONE call, one
    selector twice; the row does not change"""
    w = w2
    assert w.small(b)[0].n_digits == {1: 1, 3: 1, 5: 2}[b]
    data, row = regs_rows(w, b)
    rf = bank2.regfile(b)
    assert rf.bits == b and lib().fheram_regs_bits(rf._h) == b and not rf.state()
    rf.load(row)
    assert np.array_equal(rf.store(), row)
    idxs = [0, (1 << b) - 1, (1 << b) // 2]
    sels = [selector(w, bank2, i, b) for i in idxs]
    sels.append(sels[1])
    idxs.append(idxs[1])
    got = rf.read(sels)
    assert got.shape == (4, w.ws, w.params.glwe_len())
    oram = oram_of(w, b, row)
    okeys = w.small(b)[1]
    for k, idx in enumerate(idxs):
        want = oram.read(oaddr(w, idx, b), okeys)
        assert np.array_equal(got[k], want), (b, k, idx, np.count_nonzero(got[k] != want))
        noise = decrypts_to(w, got[k], word_of(w, data, idx), False, (b, idx))
        print(f"regs read b={b} idx={idx}: log2 noise {noise:.2f}")
    assert sha(rf.store()) == sha(row) and not rf.state(), "a read changed the register file"
    assert rf.read(sels[:2], download=False) is None
    assert np.array_equal(rf.result(0, 2), got[:2]) and np.array_equal(rf.result(1, 1)[0], got[1])


# ---- 2. pack ----------------------------------------------------------------------------------------------------------------------------------
def test_pack_then_read_equals_the_select_and_the_oracle(w2):
    """m = 5 < 2^3 candidates from HOST, ZERO and MEMBER_RESULT sources; every index, those >= m too (they read zero)"""
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    b, m = 3, 5
    bank = w.new_bank(2)
    vals, cts = w.candidates(2, seed=42)
    r0 = bank.read([w.addrs[0]], w.keys, first=0)[0]
    r1 = bank.read_prepare_write([w.addrs[1]], w.keys, first=1)[0]
    srcs = [S.host(1), S.zero(), S.member(0), S.host(0), S.member(1)]
    cand = np.stack([cts[1], np.zeros_like(r0), r0, cts[0], r1])
    rf = bank.regfile(b)
    rf.pack(srcs, host_words=cts)
    assert not rf.state()
    sels = [selector(w, bank, i, b) for i in range(1 << b)]
    got = rf.read(sels)
    via_select = bank.select(sels, [srcs] * len(sels), host_words=cts)
    assert np.array_equal(got, via_select), np.count_nonzero(got != via_select)
    for idx in range(1 << b):
        want = w.oselect(b, cand, enc_digits(w, idx, b))
        assert np.array_equal(got[idx], want), (idx, np.count_nonzero(got[idx] != want))
    noise = w.check_value(got[3], vals[0], "packed host word")
    print(f"regs pack + read: log2 noise {noise:.2f}")
    w.check_value(got[6], None, "an index past the candidates")
    # the all-zero register file, with no host encryption
    rf.pack([S.zero()] * (1 << b))
    assert not np.any(rf.store())
    assert bank.state(1) and not bank.state(0)


# ---- 3. read_prepare_write / write -------------------------------------------------------------------------------------------------------------
CONFIGS = [None, {"memo": 0}, {"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}]


@pytest.mark.parametrize("config", CONFIGS, ids=["default", "memo0", "safe_monitor2", "tail0_fuse0"])
def test_write_cycle_equals_the_oracle(w2, config):
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    b, idx = 5, 19
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=43)
    bank = w.new_bank(2, config=config)
    bank._use_keys(w.keys)
    rf = bank.regfile(b)
    rf.load(row)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    sel = selector(w, bank, idx, b)
    old = rf.read_prepare_write(sel)
    want_old = oram.read_prepare_write(oaddr(w, idx, b), okeys)
    assert np.array_equal(old, want_old), np.count_nonzero(old != want_old)
    assert np.array_equal(rf.old_result(), old)
    assert np.array_equal(rf.store(), orow(w, oram)), "the rotated row"
    assert rf.state() and oram.state
    decrypts_to(w, old, word_of(w, data, idx), False, "the old word")
    rf.write(sel, S.host(0), host_words=cts)
    oram.write(cts[0], oaddr(w, idx, b), okeys)
    assert np.array_equal(rf.store(), orow(w, oram)), "the row after the write"
    assert not rf.state() and not oram.state
    others = [0, 31]
    got = rf.read([sel] + [selector(w, bank, i, b) for i in others])
    for k, i in enumerate([idx] + others):
        want = oram.read(oaddr(w, i, b), okeys)
        assert np.array_equal(got[k], want), (i, np.count_nonzero(got[k] != want))
    noise = decrypts_to(w, got[0], vals[0], True, "the written word")
    for k, i in enumerate(others):
        noise = max(noise, decrypts_to(w, got[1 + k], word_of(w, data, i), False, ("untouched word", i)))
    print(f"regs write cycle {config}: log2 noise {noise:.2f}, round-off maximum {bank.roundoff_max():.4f}")
    assert sha(bank.store_encrypted(0)) == sha(w.rows[0]) and sha(bank.store_encrypted(1)) == sha(w.rows[1])


# ---- 4. state carried between cycles -----------------------------------------------------------------------------------------------------------
def test_three_write_cycles(w2, bank2):
    w, S = w2, w2.pkg.Src
    b = 5
    data, row = regs_rows(w, b, seed=1)
    vals, cts = w.candidates(3, seed=44)
    rf = bank2.regfile(b)
    rf.load(row)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    for k, idx in enumerate([7, 30, 7]):
        sel = selector(w, bank2, idx, b)
        assert rf.read_prepare_write(sel, download=False) is None
        oram.read_prepare_write(oaddr(w, idx, b), okeys)
        rf.write(sel, S.host(k), host_words=cts)
        oram.write(cts[k], oaddr(w, idx, b), okeys)
        assert np.array_equal(rf.store(), orow(w, oram)), ("cycle", k)
        assert not rf.state()
    got = rf.read([selector(w, bank2, i, b) for i in (7, 30)])
    noise = max(decrypts_to(w, got[0], vals[2], True), decrypts_to(w, got[1], vals[1], True))
    print(f"regs three cycles: log2 noise {noise:.2f}")


# ---- 5. every word source of a write -----------------------------------------------------------------------------------------------------------
def test_every_word_source_of_a_write(w2):
    w, pkg, S = w2, w2.pkg, w2.pkg.Src
    b = 3
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(2, seed=45)
    bank = w.new_bank(2)
    bank.read([w.addrs[0]], w.keys, first=0)
    bank.read_list([1, 0], [w.addrs[1], w.addrs[2]], w.keys, download=False)
    bank.select([selector(w, bank, 1, 1)], [[S.host(0), S.host(1)]], host_words=cts, download=False)
    rf = bank.regfile(b)
    rf.load(row)
    rf.read([selector(w, bank, 2, b), selector(w, bank, 5, b)], download=False)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    zero = np.zeros((w.ws, w.params.glwe_len()), dtype=np.int64)
    sources = [("ZERO", S.zero(), lambda: zero), ("MEMBER_RESULT", S.member(0), lambda: bank.result(0, 1)[0]),
               ("LIST_RESULT", S.list(1), lambda: bank.list_result(1, 1)[0]), ("SELECT_RESULT", S.select(0), lambda: bank.select_result(0, 1)[0]),
               ("REGS_RESULT", S.regs(1), lambda: rf.result(1, 1)[0]), ("REGS_OLD", S.regs_old(), lambda: rf.old_result())]
    for k, (name, src, fetch) in enumerate(sources):
        idx = (3 * k + 1) % (1 << b)
        sel = selector(w, bank, idx, b)
        rf.read_prepare_write(sel, download=False)
        oram.read_prepare_write(oaddr(w, idx, b), okeys)
        rf.write(sel, src)
        oram.write(fetch(), oaddr(w, idx, b), okeys)
        assert np.array_equal(rf.store(), orow(w, oram)), name
        assert not rf.state(), name
    w.check_value(rf.read([selector(w, bank, 1, b)])[0], None, "the word ZERO was written to")


# ---- 6. the write enable ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enable", [0, 1])
def test_write_enable_without_a_sync(w2, bank2, enable):
    """rd <- enable ? new : old, all on the device: read_prepare_write, a select over [REGS_OLD, HOST] by a 1-bit selector, write(SELECT_RESULT)"""
    w, S = w2, w2.pkg.Src
    b, rd = 3, 6
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=46)
    rf = bank2.regfile(b)
    rf.load(row)
    sel, en = selector(w, bank2, rd, b), selector(w, bank2, enable, 1)
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
    got = rf.read([selector(w, bank2, i, b) for i in range(1 << b)])
    noise = -1e9
    for i in range(1 << b):
        if i != rd:
            noise = max(noise, decrypts_to(w, got[i], word_of(w, data, i), False, ("untouched", i)))
        elif enable:
            noise = max(noise, decrypts_to(w, got[i], vals[0], True, "the new word"))
        else:   # the old value, as the register file held it
            noise = max(noise, decrypts_to(w, got[i], word_of(w, data, i), False, "the old word kept"))
    print(f"regs write enable = {enable}: log2 noise {noise:.2f}")


# ---- 7. lanes out of register results ---------------------------------------------------------------------------------------------------------
def test_select_lanes_takes_lanes_from_register_results(po):
    w = LaneWorld(po, 1 << 12, 2, 4, seed=420)
    pkg, L = w.pkg, w.pkg.Lane
    b = 3
    data, row = regs_rows(w, b)
    bank = w.new_bank(2)
    bank._use_keys(w.keys)
    rf = bank.regfile(b)
    rf.load(row)
    r = rf.read([selector(w, bank, 2, b), selector(w, bank, 7, b)])
    rf.read_prepare_write(selector(w, bank, 4, b), download=False)
    old = rf.old_result()
    cands = [[L.regs(0, 0), L.regs(1, 1), L.zero(), L.regs(0, 3)], [L.regs(1, 3 - l) for l in range(4)], [L.regs_old(l) for l in (1, 0, 3, 2)]]
    words = w.assemble(cands, {(5, 0): r[0], (5, 1): r[1], (6, 0): old})
    for idx in range(3):
        sel = selector(w, bank, idx, 2)
        got = bank.select_lanes([sel], [cands])[0]
        host = bank.select([sel], [[pkg.Src.host(j) for j in range(3)]], host_words=words)[0]
        assert np.array_equal(got, host), (idx, np.count_nonzero(got != host))
        assert np.array_equal(got, w.oselect(2, words, enc_digits(w, idx, 2))), idx
    assert rf.state()


# ---- 8. selectors out of one derive list ------------------------------------------------------------------------------------------------------
def test_rs1_rs2_rd_from_one_instruction_word(w2, bank2):
    """rs1 = bits [15, 20), rs2 = [20, 25), rd = [7, 12) of one encrypted integer, derived in ONE launch; then the reads and the register write"""
    w, pkg, S, D = w2, w2.pkg, w2.pkg.Src, w2.pkg.Derive
    b = 5
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(1, seed=47)
    fu = pkg.FheUintPrepared.from_host(bank2, w.bits(VALUE))
    rs1, rs2, rd = (bank2.selector(b) for _ in range(3))
    bank2.derive_list([D.selector(fu, rs1, 15), D.selector(fu, rs2, 20), D.selector(fu, rd, 7)])
    rf = bank2.regfile(b)
    rf.load(row)
    got = rf.read([rs1, rs2], download=False)
    rf.read_prepare_write(rd, download=False)
    rf.write(rd, S.host(0), host_words=cts)
    i1, i2, i3 = ((VALUE >> f) & 31 for f in (15, 20, 7))
    ob, okeys = w.small(b)
    oram = oram_of(w, b, row)
    a1, a2, a3 = (ob.address_new(w.digits(VALUE, f, b)) for f in (15, 20, 7))
    got = rf.result(0, 2)
    assert np.array_equal(got[0], oram.read(a1, okeys)) and np.array_equal(got[1], oram.read(a2, okeys))
    noise = max(decrypts_to(w, got[0], word_of(w, data, i1), False, "rs1"), decrypts_to(w, got[1], word_of(w, data, i2), False, "rs2"))
    assert np.array_equal(rf.old_result(), oram.read_prepare_write(a3, okeys))
    oram.write(cts[0], a3, okeys)
    assert np.array_equal(rf.store(), orow(w, oram))
    noise = max(noise, decrypts_to(w, rf.read([rd])[0], vals[0], True, "rd"))
    print(f"regs step from derived selectors (rs1 = {i1}, rs2 = {i2}, rd = {i3}): log2 noise {noise:.2f}")


# ---- 9. isolation ------------------------------------------------------------------------------------------------------------------------------
def test_a_register_write_cycle_inside_a_members_write(w13):
    """at 2^13 (two rows, two coordinates): member 0 sits between read_prepare_write and write while a register file is read, prepared and written"""
    w, S = w13, w13.pkg.Src
    b = 5
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(3, seed=48)
    bank = w.new_bank(2)
    a = w.addrs
    lst = bank.read_list([1, 0], [a[1], a[2]], w.keys)
    picked = bank.select([selector(w, bank, 1, 1)], [[S.host(0), S.list(0)]], host_words=cts)
    bank.read_prepare_write([a[0]], w.keys, first=0)
    before = (sha(bank.list_result(0, 2)), sha(bank.select_result(0, 1)), sha(bank.result(0, 2)), sha(bank.tree(0, 0)), sha(bank.store_encrypted(1)))
    rf = bank.regfile(b)
    rf.load(row)
    oram, okeys = oram_of(w, b, row), w.small(b)[1]
    sel = selector(w, bank, 11, b)
    got = rf.read([sel, selector(w, bank, 3, b)], download=False)
    rf.read_prepare_write(sel, download=False)
    rf.write(sel, S.host(2), host_words=cts)
    oram.read_prepare_write(oaddr(w, 11, b), okeys)
    oram.write(cts[2], oaddr(w, 11, b), okeys)
    assert np.array_equal(rf.store(), orow(w, oram))
    assert [bank.state(0), bank.state(1)] == [True, False]
    after = (sha(bank.list_result(0, 2)), sha(bank.select_result(0, 1)), sha(bank.result(0, 2)), sha(bank.tree(0, 0)), sha(bank.store_encrypted(1)))
    assert after == before, "a register operation moved something of the bank"
    assert np.array_equal(bank.list_result(0, 2), lst) and np.array_equal(bank.select_result(0, 1), picked)
    # the member resumes its write exactly as the oracle's RAM does
    om = w.new_oram(0)
    om.read_prepare_write(w.o.address_new(w.addr_g[0]), w.okeys)
    om.write(cts[1], w.o.address_new(w.addr_g[0]), w.okeys)
    bank.write(cts[1:2], [a[0]], w.keys, first=0)
    assert np.array_equal(bank.store_encrypted(0), om.store()), np.count_nonzero(bank.store_encrypted(0) != om.store())
    assert not bank.state(0)


# ---- 10. refusals, two register files, lifetimes ------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(w2, w13):
    w, pkg, S, Ln = w2, w2.pkg, w2.pkg.Src, w2.pkg.Lane
    L = lib()
    b = 3
    data, row = regs_rows(w, b)
    vals, cts = w.candidates(2, seed=49)
    bank, other, fresh = w.new_bank(2), w13.new_bank(1), w.new_bank(2)   # fresh: keys not loaded
    bank._use_keys(w.keys)
    other._use_keys(w13.keys)
    rf, rf_other, rf_fresh, rf_empty = bank.regfile(b), other.regfile(b), fresh.regfile(b), bank.regfile(b)
    for r in (rf, rf_other, rf_fresh):
        r.load(row)
    sel, sel5, empty = selector(w, bank, 2, b), selector(w, bank, 2, 5), bank.selector(b)
    foreign = selector(w13, other, 2, b)
    en = selector(w, bank, 1, 1)

    def digest():
        return sha(rf.store()), rf.state(), [sha(bank.store_encrypted(m)) for m in range(2)]

    def refused(code, call, what):
        before = digest()
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg, what
        assert digest() == before, what

    refused(ST_INVALID_ARG, lambda: bank.regfile(0), "bits 0")
    refused(ST_INVALID_ARG, lambda: bank.regfile(6), "bits 6")
    assert L.fheram_bank_regs_create(bank._h, b, None) == ST_INVALID_ARG and L.fheram_bank_regs_create(None, b, None) == ST_INVALID_ARG
    # -- before any register read / read_prepare_write of the bank
    refused(ST_STATE, lambda: rf.result(0, 1), "result before any read")
    refused(ST_STATE, lambda: rf.old_result(), "old_result before any read_prepare_write")
    refused(ST_STATE, lambda: bank.select([en], [[S.regs(0), S.zero()]]), "REGS_RESULT before any register read")
    refused(ST_STATE, lambda: bank.select([en], [[S.regs_old(), S.zero()]]), "REGS_OLD before any read_prepare_write")
    refused(ST_STATE, lambda: rf.pack([S.regs(0)]), "pack from REGS_RESULT before any register read")
    # -- unknown kinds stay unknown: 7 in select, lanes, pack and write
    refused(ST_INVALID_ARG, lambda: bank.select([en], [[S(7, 0), S.zero()]]), "kind 7 in select")
    refused(ST_INVALID_ARG, lambda: bank.select_lanes([en], [[[Ln(7, 0, 0)] * w.ws, [Ln.zero()] * w.ws]]), "kind 7 in select_lanes")
    refused(ST_INVALID_ARG, lambda: rf.pack([S(7, 0)]), "kind 7 in pack")
    # -- read
    refused(ST_INVALID_ARG, lambda: rf.read([sel5]), "a selector of other bits")
    refused(ST_INVALID_ARG, lambda: rf.read([empty]), "an empty selector")
    refused(ST_INVALID_ARG, lambda: rf.read([foreign]), "a selector of another bank")
    refused(ST_INVALID_ARG, lambda: rf.read([sel] * 9), "n = 9")
    refused(ST_UNINITIALIZED, lambda: rf_empty.read([sel]), "no upload or pack yet")
    refused(ST_UNINITIALIZED, lambda: rf_empty.store(), "download before any upload")
    refused(ST_UNINITIALIZED, lambda: rf_empty.read_prepare_write(sel), "read_prepare_write before any upload")
    p1 = (C.c_void_p * 1)(sel._h)
    assert L.fheram_bank_regs_read(bank._h, rf._h, None, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_read(bank._h, None, p1, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_read(None, rf._h, p1, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_read(bank._h, rf._h, p1, 0, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_read(bank._h, rf_other._h, p1, 1, None) == ST_INVALID_ARG   # a register file of another bank
    assert L.fheram_bank_regs_upload(bank._h, rf._h, None) == ST_INVALID_ARG and L.fheram_bank_regs_download(bank._h, rf._h, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_upload(bank._h, rf_other._h, row.ctypes.data_as(I64P)) == ST_INVALID_ARG
    assert L.fheram_bank_regs_pack(bank._h, rf._h, 1, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_read_prepare_write(bank._h, rf._h, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_write(bank._h, rf._h, None, pkg.api._CSelectSrc(0, 0), None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_result(bank._h, 0, 1, None) == ST_INVALID_ARG and L.fheram_bank_regs_old_result(bank._h, None) == ST_INVALID_ARG
    assert L.fheram_bank_regs_state(bank._h, rf_other._h) == 0 and L.fheram_bank_regs_state(None, rf._h) == 0 and L.fheram_regs_bits(None) == 0
    refused(ST_KEYS, lambda: rf_fresh.read([selector(w, fresh, 2, b)]), "keys not loaded")
    bad = cts.copy()
    bad[0, 1, 9] = -(1 << 16) - 1
    refused(ST_RANGE, lambda: rf.load(np.full_like(row, 1 << 17)), "an upload out of range")
    refused(ST_RANGE, lambda: rf.pack([S.host(0)], host_words=bad), "a packed host limb out of range")
    refused(ST_INVALID_ARG, lambda: rf.pack([S.host(0)]), "HOST without host_words")
    refused(ST_INVALID_ARG, lambda: rf.pack([S.zero()] * 9), "n_cand > 2^bits")
    refused(ST_INVALID_ARG, lambda: rf.pack([S.member(2)]), "member outside the bank")
    refused(ST_STATE, lambda: rf.pack([S.member(1)]), "a member without a result")
    # -- state 0: no write; a valid read behind the refusals
    refused(ST_STATE, lambda: rf.write(sel, S.zero()), "write in state 0")
    first = rf.read([sel])[0]
    refused(ST_INVALID_ARG, lambda: rf.result(1, 1), "result outside the last read")
    refused(ST_INVALID_ARG, lambda: bank.select([en], [[S.regs(1), S.zero()]]), "REGS_RESULT outside the last read")
    refused(ST_INVALID_ARG, lambda: bank.select([en], [[S(6, 1), S.zero()]], keys=w.keys), "REGS_OLD with index 1")
    # -- state 1: read, pack and read_prepare_write are refused, a refused word leaves the register file prepared; upload resets
    old = rf.read_prepare_write(sel)
    assert np.array_equal(old, first), "read_prepare_write returns what a read returns"
    refused(ST_STATE, lambda: rf.read([sel]), "read in state 1")
    refused(ST_STATE, lambda: rf.pack([S.zero()]), "pack in state 1")
    refused(ST_STATE, lambda: rf.read_prepare_write(sel), "read_prepare_write in state 1")
    refused(ST_RANGE, lambda: rf.write(sel, S.host(0), host_words=bad), "a written host limb out of range")
    refused(ST_INVALID_ARG, lambda: rf.write(sel, S(7, 0)), "kind 7 in write")
    refused(ST_INVALID_ARG, lambda: rf.write(sel, S.host(0)), "HOST without host_words")
    refused(ST_INVALID_ARG, lambda: rf.write(sel5, S.zero()), "a selector of other bits")
    refused(ST_INVALID_ARG, lambda: rf.write(foreign, S.zero()), "a selector of another bank")
    assert rf.state()
    # two register files on one bank: the second's whole cycle runs inside the first's, new keys are loaded between the halves
    rf2 = bank.regfile(5)
    data5, row5 = regs_rows(w, 5)
    rf2.load(row5)
    o2, okeys5 = oram_of(w, 5, row5), w.small(5)[1]
    s2 = selector(w, bank, 9, 5)
    rf2.read_prepare_write(s2, download=False)
    assert np.array_equal(rf2.old_result(), o2.read_prepare_write(oaddr(w, 9, 5), okeys5)), "REGS_OLD is now the second file's"
    rf2.write(s2, S.host(1), host_words=cts)
    o2.write(cts[1], oaddr(w, 9, 5), okeys5)
    assert np.array_equal(rf2.store(), orow(w, o2)) and rf.state() and not rf2.state()
    bank._keys = None
    bank._use_keys(w.keys)   # fheram_bank_keys_load: what the first file kept is void, its write recomputes it
    rf.write(sel, S.host(0), host_words=cts)
    o1, okeys = oram_of(w, b, row), w.small(b)[1]
    o1.read_prepare_write(oaddr(w, 2, b), okeys)
    o1.write(cts[0], oaddr(w, 2, b), okeys)
    assert np.array_equal(rf.store(), orow(w, o1)) and not rf.state()
    # upload between the halves resets, as fheram_bank_ram_upload does
    rf.read_prepare_write(sel, download=False)
    rf.load(row)
    assert not rf.state() and np.array_equal(rf.read([sel])[0], first)
    # lifetimes: the register file whose read_prepare_write was the last takes REGS_OLD with it; a bank destroyed first leaves handles that
    # only fheram_regs_destroy may take, and takes
    rf.read_prepare_write(sel, download=False)
    h = rf._h
    rf._h = None
    L.fheram_regs_destroy(h)
    refused_code = L.fheram_bank_regs_old_result(bank._h, old.ctypes.data_as(I64P))
    assert refused_code == ST_STATE
    hb, h2 = other._h, rf_other._h
    other._h = None
    rf_other._h = None
    L.fheram_bank_destroy(hb)
    assert L.fheram_regs_bits(h2) == b
    L.fheram_regs_destroy(h2)
    L.fheram_regs_destroy(None)
    assert np.array_equal(rf2.read([s2])[0], o2.read(oaddr(w, 9, 5), okeys5)), "the bank and its other register file still work"
