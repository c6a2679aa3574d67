"""fheram_bank_read_prepare_write_list / fheram_bank_write_list (RamBank.read_prepare_write_list / write_list): read_prepare_write and
write on ANY set of distinct members of a bank — any order, any subset — as ONE operation each (include/fheram.h).

The contract: the calls are int64-identical to the n single-member calls; every named member is afterwards — state flag, rows, tree level
0, result — where a standalone Ram loaded with the same keys and rows and driven the same way is; members that are not named are untouched
in every respect; lists, ranges and single calls mix freely between the two halves; a refused call changes nothing.  No tolerance
anywhere: every comparison is np.array_equal on int64."""
import ctypes as C

import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import CLASSES, World, assert_member_is, lib, member_snapshot, profiled

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS, ST_RANGE, ST_DEVICE = 1, 2, 3, 4, 6, 7
I64P = C.POINTER(C.c_int64)
J = [1, 3, 0, 2]      # the address of member m: a different one per member, so per entry of any list
WORDS_SEED = 5
_STANDALONE = {}


def has_tree(w):
    return w.max_addr > 4096   # one coordinate: the rows are the tree


def snap(w, owner, m=None):
    """(rows, tree level 0 or None, state) of a bank member or of a standalone Ram"""
    if m is None:
        return owner.store_encrypted(), owner.tree(0) if has_tree(w) else None, bool(owner.state)
    return owner.store_encrypted(m), owner.tree(m, 0) if has_tree(w) else None, owner.state(m)


def assert_snap(got, want, what):
    assert got[2] == want[2], (what, "state")
    assert np.array_equal(np.ravel(got[0]), np.ravel(want[0])), (what, "rows")
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "tree")


def words_of(w):
    if not hasattr(w, "_wl_words"):
        w._wl_words = w.words(w.M, seed=WORDS_SEED)
    return w._wl_words


def standalone(w, m, j=None):
    """the flow of ONE standalone Ram (default switches) holding member m's rows: read_prepare_write at address j, write of member m's
    words, read-back — computed once per (world, member, address) and shared by every test"""
    j = J[m] if j is None else j
    key = (id(w), m, j)
    if key not in _STANDALONE:
        ram, a = w.new_ram(m), w.addrs[j]
        out = {"rpw": ram.read_prepare_write(a, w.keys).copy()}
        out["result_after_rpw"] = ram.result().copy()
        out["after_rpw"] = snap(w, ram)
        ram.write(words_of(w)[1][m], a, w.keys)
        out["after_write"] = snap(w, ram)
        out["readback"] = ram.read(a, w.keys).copy()
        _STANDALONE[key] = out
    return _STANDALONE[key]


def addrs_of(w, members):
    return [w.addrs[J[m]] for m in members]


def rpw_list(w, bank, members, **kw):
    return bank.read_prepare_write_list(members, addrs_of(w, members), w.keys, **kw)


def write_list(w, bank, members):
    bank.write_list(members, np.stack([words_of(w)[1][m] for m in members]), addrs_of(w, members), w.keys)


def check_prepared(w, bank, members, got, what=""):
    if got is not None:
        assert got.shape == (len(members), w.ws, w.params.glwe_len())
    for k, m in enumerate(members):
        want = standalone(w, m)
        if got is not None:
            assert np.array_equal(got[k], want["rpw"]), (what, "slice", k, m, np.count_nonzero(got[k] != want["rpw"]))
        assert_snap(snap(w, bank, m), want["after_rpw"], (what, "after read_prepare_write", m))
        assert np.array_equal(bank.result(m, 1)[0], want["result_after_rpw"]), (what, "result", m)


def check_written(w, bank, members, what="", readback=True):
    for m in members:
        assert_snap(snap(w, bank, m), standalone(w, m)["after_write"], (what, "after write", m))
    if readback:
        got = bank.read_list(members, addrs_of(w, members), w.keys)
        for k, m in enumerate(members):
            assert np.array_equal(got[k], standalone(w, m)["readback"]), (what, "read-back", k, m)


def full_flow(w, bank, members, write_order=None, what=""):
    others = {m: snap(w, bank, m) for m in range(len(bank)) if m not in members}
    got = rpw_list(w, bank, members)
    check_prepared(w, bank, members, got, what)
    for m, s in others.items():
        assert_snap(snap(w, bank, m), s, (what, "not named, after read_prepare_write", m))
    write_list(w, bank, write_order or members)
    check_written(w, bank, members, what)
    for m, s in others.items():
        assert_snap(snap(w, bank, m), s, (what, "not named, after write", m))


@pytest.fixture(scope="module")
def w14(po):
    return World(po, 1 << 14, 3, n_addr=4)


@pytest.fixture(scope="module")
def w16(po):
    """2^16: 16 rows, coordinate 1 has two digits: the fused row chains, k_trace_tail_t at n * ws <= 8, the mid chain above it"""
    return World(po, 1 << 16, 4, seed=80, n_addr=4)


# ---- 1. plain lists ----------------------------------------------------------------------------------------------------------------------
PLAIN = [([0], None), ([2, 0], None), ([2, 0], [0, 2]), ([0, 2], None), ([0, 2], [2, 0]), ([1, 2], None), ([1, 2], [2, 1]),
         ([2, 1, 0], None), ([2, 1, 0], [1, 0, 2])]


@pytest.mark.parametrize("members,write_order", PLAIN, ids=["".join(map(str, m)) + ("" if o is None else "-w" + "".join(map(str, o))) for m, o in PLAIN])
def test_lists_equal_standalone_rams_2_14(w14, members, write_order):
    full_flow(w14, w14.new_bank(3), members, write_order, (members, write_order))


def test_list_equals_the_oracle_2_14(w14):
    w = w14
    members = [2, 0]
    bank = w.new_bank(3)
    vals, wct = words_of(w)
    got = rpw_list(w, bank, members)
    orams = {}
    for k, m in enumerate(members):
        orams[m], oa = w.new_oram(m), w.o.address_new(w.addr_g[J[m]])
        assert np.array_equal(got[k], orams[m].read_prepare_write(oa, w.okeys)), m
        w.check_word(got[k], w.data[m], J[m])
        assert np.array_equal(bank.tree(m, 0), orams[m].tree(0)), m
    write_list(w, bank, members)
    back = bank.read_list(members, addrs_of(w, members), w.keys)
    for k, m in enumerate(members):
        oa = w.o.address_new(w.addr_g[J[m]])
        orams[m].write(wct[m], oa, w.okeys)
        assert np.array_equal(bank.store_encrypted(m), orams[m].store()), m
        assert np.array_equal(bank.tree(m, 0), orams[m].tree(0)), m
        assert np.array_equal(back[k], orams[m].read(oa, w.okeys)), m
        data2 = w.data[m].copy()
        data2[w.ws * w.idx[J[m]]: w.ws * (w.idx[J[m]] + 1)] = vals[m]
        w.check_word(back[k], data2, J[m], written=True)


# ---- 2. mixing prepared members ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memo", [1, 0])
def test_lists_ranges_and_single_calls_mix_2_14(w14, memo):
    w = w14
    vals, wct = words_of(w)
    cfg = {"memo": memo}
    # a list prepares; a range of one and a list of one write
    bank = w.new_bank(3, config=cfg)
    check_prepared(w, bank, [2, 0], rpw_list(w, bank, [2, 0]), "list, then singles")
    bank.write(wct[0:1], [w.addrs[J[0]]], w.keys, first=0)
    assert [bank.state(m) for m in range(3)] == [False, False, True]
    write_list(w, bank, [2])
    check_written(w, bank, [0, 2], "list, then singles")
    assert_snap(snap(w, bank, 1), (w.rows[1], None, False), "member 1")
    # a range prepares; a list writes, in the other order
    bank = w.new_bank(3, config=cfg)
    got = bank.read_prepare_write(addrs_of(w, [0, 1]), w.keys, first=0)
    check_prepared(w, bank, [0, 1], got, "range, then list")
    write_list(w, bank, [1, 0])
    check_written(w, bank, [0, 1], "range, then list")
    # a list and a single call prepare; one list writes all three
    bank = w.new_bank(3, config=cfg)
    check_prepared(w, bank, [0, 2], rpw_list(w, bank, [0, 2]), "list + single, then list")
    got = bank.read_prepare_write([w.addrs[J[1]]], w.keys, first=1)
    check_prepared(w, bank, [1], got, "list + single, then list")
    check_prepared(w, bank, [0, 2], None, "list + single, then list: the list's members behind the single call")
    write_list(w, bank, [1, 2, 0])
    check_written(w, bank, [0, 1, 2], "list + single, then list")


# ---- 3. members that are not named are untouched -----------------------------------------------------------------------------------------
def test_a_pending_member_and_the_last_read_list_survive_2_14(w14):
    w = w14
    vals, wct = words_of(w)
    bank = w.new_bank(3)
    last = bank.read_list([0, 2], [w.addrs[2], w.addrs[3]], w.keys).copy()
    a1 = w.addrs[J[1]]
    check_prepared(w, bank, [1], bank.read_prepare_write([a1], w.keys, first=1), "member 1 alone")
    s1 = snap(w, bank, 1)
    check_prepared(w, bank, [2, 0], rpw_list(w, bank, [2, 0]), "beside a pending member")
    assert_snap(snap(w, bank, 1), s1, "member 1 across the read_prepare_write list")
    assert np.array_equal(bank.list_result(0, 2), last)
    write_list(w, bank, [0, 2])
    assert_snap(snap(w, bank, 1), s1, "member 1 across the write list")
    assert np.array_equal(bank.result(1, 1)[0], standalone(w, 1)["result_after_rpw"])
    assert np.array_equal(bank.list_result(0, 2), last)
    assert [bank.state(m) for m in range(3)] == [False, True, False]
    bank.write(wct[1:2], [a1], w.keys, first=1)           # member 1's own write resumes from what it kept
    check_written(w, bank, [0, 1, 2], "behind the lists")


def test_a_read_list_between_the_two_halves_changes_nothing_2_14(w14):
    w = w14
    bank = w.new_bank(3)
    check_prepared(w, bank, [2, 0], rpw_list(w, bank, [2, 0]), "first half")
    s1 = snap(w, bank, 1)
    twin = w.new_bank(3)
    want = twin.read_list([1, 1], [w.addrs[0], w.addrs[2]], w.keys)
    got = bank.read_list([1, 1], [w.addrs[0], w.addrs[2]], w.keys)
    assert np.array_equal(got, want)
    check_prepared(w, bank, [2, 0], None, "behind the read list")
    write_list(w, bank, [0, 2])
    check_written(w, bank, [0, 2], "second half", readback=False)
    assert_snap(snap(w, bank, 1), s1, "member 1")
    assert np.array_equal(bank.list_result(0, 2), want)
    check_written(w, bank, [0, 2], "second half")


def test_key_reload_between_the_two_halves_2_14(w14):
    """fheram_bank_keys_load voids everything a read_prepare_write kept: the write recomputes it, and the outcome is the same"""
    w = w14
    bank = w.new_bank(3)
    check_prepared(w, bank, [2, 0], rpw_list(w, bank, [2, 0]), "first half")
    bank._keys = None
    bank._use_keys(w.keys)
    write_list(w, bank, [2, 0])
    check_written(w, bank, [2, 0], "behind a key reload")


# ---- 4. forced forms -------------------------------------------------------------------------------------------------------------------------
FORMS = [{"tail": 0}, {"tail_ep": 0}, {"mid": 0}, {"fuse": 0}, {"chain": 0}, {"safe": 1}, {"graph": 1}, {"memo": 0}, {"tail_test": 1}, {"mid_test": 1}]


@pytest.mark.parametrize("config", FORMS, ids=["-".join(f"{k}{v}" for k, v in c.items()) for c in FORMS])
@pytest.mark.parametrize("size", [14, 16])
def test_forced_forms_equal_the_default_form(w14, w16, size, config):
    """every observable of the list [2, 0] and its write equals the standalone Ram's in the default forms"""
    w = w14 if size == 14 else w16
    full_flow(w, w.new_bank(3, config=config), [2, 0], None, (size, config))


# ---- 5. the launches that should run, do ---------------------------------------------------------------------------------------------------
def test_list_launch_profile_2_16(w16):
    """[2, 0] at ws = 4 is 8 ciphertexts: the rows' chains of both entries are ONE mapped read chain / write chain launch on the members'
    own rows, and the end of read_prepare_write ONE k_trace_tail_t that does not give up.  [3, 1, 0] ends in the mid chain."""
    w = w16
    rows = w.params.rows()
    members = [2, 0]
    bank = w.new_bank(3)
    t0 = bank.tail_stats()
    got, prof = profiled(bank, lambda: rpw_list(w, bank, members), CLASSES)
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * 2 * w.ws, prof
    assert prof["keyswitch_tail_launch"]["launches"] == 1 and prof["keyswitch_mid_launch"]["launches"] == 0, prof
    t1 = bank.tail_stats()
    assert t1["launches"] == t0["launches"] + 1 and t1["fallbacks"] == t0["fallbacks"], (t0, t1)
    check_prepared(w, bank, members, got, "2^16")
    _, prof = profiled(bank, lambda: write_list(w, bank, members), CLASSES)
    assert prof["write_chain_launch"]["launches"] == 1 and prof["write_chain_launch"]["blocks"] == rows * 2 * w.ws, prof
    assert prof["read_chain_launch"]["launches"] == 0, prof
    check_written(w, bank, members, "2^16")
    assert_snap(snap(w, bank, 1), (w.rows[1], None, False), "member 1")
    members = [3, 1, 0]
    bank = w.new_bank(4)
    t0 = bank.tail_stats()
    got, prof = profiled(bank, lambda: rpw_list(w, bank, members), CLASSES)
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * 3 * w.ws, prof
    assert prof["keyswitch_mid_launch"]["launches"] >= 1 and prof["keyswitch_tail_launch"]["launches"] == 0, prof
    check_prepared(w, bank, members, got, "2^16, three entries")
    _, prof = profiled(bank, lambda: write_list(w, bank, members), CLASSES)
    assert prof["write_chain_launch"]["launches"] == 1 and prof["write_chain_launch"]["blocks"] == rows * 3 * w.ws, prof
    check_written(w, bank, members, "2^16, three entries")
    ms = bank.mid_stats()
    assert ms["launches"] > 0 and ms["fallbacks"] == 0, ms
    assert bank.tail_stats()["launches"] == t0["launches"]


# ---- 6. one row, two rows, 5-limb trace keys -----------------------------------------------------------------------------------------------
SMALL = [(12, 4, {}), (12, 2, {}), (13, 4, {}), (13, 2, {}), (14, 4, {"k_glwe_pt": 9, "k_evk_trace": 85})]


@pytest.mark.parametrize("size,ws,crypto", SMALL, ids=["2p12", "2p12-ws2", "2p13", "2p13-ws2", "2p14-readme"])
def test_one_row_two_rows_and_readme_keys(po, size, ws, crypto):
    """2^12: one row, one coordinate (n2 == 1: the member's row is the tree top, every launch on it goes member by member); 2^13: two rows
    (at word size 2 the alone levels of the list run as the tail chain); the README block: the <5, 4> instantiations of the mapped chains"""
    w = World(po, 1 << size, 3, word_size=ws, seed=300 + size + ws, n_addr=4, **crypto)
    full_flow(w, w.new_bank(3), [2, 0], None, (size, ws))
    for m in (0, 2):
        data2 = w.data[m].copy()
        data2[w.ws * w.idx[J[m]]: w.ws * (w.idx[J[m]] + 1)] = words_of(w)[0][m]
        w.check_word(standalone(w, m)["readback"], data2, J[m], written=True)
    for key in [k for k in _STANDALONE if k[0] == id(w)]:
        del _STANDALONE[key]


# ---- 7. enqueue only ---------------------------------------------------------------------------------------------------------------------------
def test_derive_and_both_lists_without_a_sync_2_14(w14):
    """fheram_bank_address_derive, the read_prepare_write list (out == NULL) and the write list, nothing between them waits for the device;
    against a twin bank that derives the same addresses, waits, and runs single-member operations"""
    w = w14
    pkg = w.pkg
    vals, wct = words_of(w)
    members = [2, 0]
    bank, twin = w.new_bank(3), w.new_bank(3)
    for b in (bank, twin):
        b.read([w.addrs[0]], w.keys, first=1)   # (loads the keys)

    def derived(b):
        fus = [pkg.FheUintPrepared.from_host(b, w.o.fheuint_encrypt(w.idx[J[m]], 14, w.sk, 6300 + 2 * k, 6301 + 2 * k)) for k, m in enumerate(members)]
        return b.derive_addresses(fus)

    addrs = derived(bank)
    assert bank.read_prepare_write_list(members, addrs, w.keys, download=False) is None
    bank.write_list(members, np.stack([wct[m] for m in members]), addrs, w.keys)
    t_addrs = derived(twin)
    twin.sync()
    for k, m in enumerate(members):
        want = twin.read_prepare_write([t_addrs[k]], w.keys, first=m)[0]
        assert np.array_equal(bank.result(m, 1)[0], want), m
        twin.write(wct[m:m + 1], [t_addrs[k]], w.keys, first=m)
    for m in range(3):
        assert_snap(snap(w, bank, m), snap(w, twin, m), ("no sync", m))
    back = bank.read_list(members, addrs, w.keys)
    for k, m in enumerate(members):
        data2 = w.data[m].copy()
        data2[w.ws * w.idx[J[m]]: w.ws * (w.idx[J[m]] + 1)] = vals[m]
        w.check_word(back[k], data2, J[m], written=True)


# ---- 8. extreme limbs through both mapped chains -------------------------------------------------------------------------------------------
def test_extreme_limbs_through_the_mapped_chains_2_16():
    """Limbs at the ends of the normalised range (tests/test_gpu_extremes_table.py: a different kind per member, address and word, so that
    a row, a digit or a word taken from the wrong member shows) through the list [2, 0] of a bank of three at 2^16: ONE mapped read chain
    and ONE mapped write chain, every coefficient monitored.  Equal to the standalone contexts; the round-off stays under the monitor's limit."""
    from test_gpu_extremes_table import gpu_keys, note_roundoff, operand, params16
    pkg = load_package()
    ws, cfg, keys_kind = 4, {"monitor": 2}, "signs"
    member_rows = ["lo", "signs", "alternating"]
    members, addr_ks, word_ks = [2, 0], ["hi", "alternating"], ["alternating", "hi"]
    p = params16(ws)
    rows = p.rows()
    keys = gpu_keys(keys_kind)
    bank = pkg.RamBank(p, 3, 0, config=cfg)
    for m, k in enumerate(member_rows):
        bank.load_encrypted(m, operand("rows", k, ws))
    A = [pkg.Address(p, list(operand("addr", k))) for k in addr_ks]
    W = np.stack([operand("words", k, ws) for k in word_ks])
    got, prof = profiled(bank, lambda: bank.read_prepare_write_list(members, A, keys), CLASSES)
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * 2 * ws, prof
    rams = []
    for k, m in enumerate(members):
        ram = pkg.Ram(p, 0, config=cfg)
        ram.load_encrypted(operand("rows", member_rows[m], ws))
        assert np.array_equal(got[k], ram.read_prepare_write(A[k], keys)), (k, m)
        assert np.array_equal(bank.store_encrypted(m), ram.store_encrypted()) and np.array_equal(bank.tree(m, 0), ram.tree(0)), (k, m)
        rams.append(ram)
    assert not np.array_equal(got[0], got[1])
    _, prof = profiled(bank, lambda: bank.write_list(members, W, A, keys), CLASSES)
    assert prof["write_chain_launch"]["launches"] == 1 and prof["write_chain_launch"]["blocks"] == rows * 2 * ws, prof
    for k, m in enumerate(members):
        rams[k].write(W[k], A[k], keys)
        assert np.array_equal(bank.store_encrypted(m), rams[k].store_encrypted()), (k, m)
        assert np.array_equal(bank.tree(m, 0), rams[k].tree(0)) and bank.state(m) is False, (k, m)
    assert np.array_equal(bank.store_encrypted(1), operand("rows", member_rows[1], ws)) and bank.state(1) is False
    back = bank.read_list(members, A, keys)
    for k in range(2):
        assert np.array_equal(back[k], rams[k].read(A[k], keys)), k
    note_roundoff(bank, f"write lists {members} of {member_rows} at {addr_ks}")


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refused_lists_change_nothing_2_14(w14):
    w = w14
    pkg = w.pkg
    L = lib()
    M = 3
    vals, wct = words_of(w)
    bank = w.new_bank(M)
    last = bank.read_list([0, 1], [w.addrs[0], w.addrs[1]], w.keys).copy()
    h = [w.addrs[J[m]]._bank(bank) for m in range(M)]
    buf = np.zeros((M, w.ws, w.params.glwe_len()), dtype=np.int64)
    RPW, WR = L.fheram_bank_read_prepare_write_list, L.fheram_bank_write_list

    def c_list(fn, members, handles, n=None, on=None, data=buf):
        n = len(members) if n is None else n
        ms = (C.c_int * max(1, len(members)))(*members)
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        return fn((on or bank)._h, ms, arr, n, data.ctypes.data_as(I64P) if data is not None else None)

    def unchanged(what, b=bank):
        assert L.fheram_bank_last_error(b._h), what
        for m in range(M):
            assert_member_is(b, m, snaps[m], what)
        assert np.array_equal(b.list_result(0, 2), last), what

    def msg():
        return L.fheram_bank_last_error(bank._h)

    def argument_refusals(fn, members):
        """what both calls refuse for their arguments alone; `members` is a list the call would accept"""
        hs = [h[m] for m in members]
        assert c_list(fn, members, hs, n=0) == ST_INVALID_ARG and b"outside [1" in msg()
        assert c_list(fn, [0, 1, 2, 0], [h[0], h[1], h[2], h[0]]) == ST_INVALID_ARG and b"outside [1" in msg()      # n > M
        assert c_list(fn, [members[0], -1], hs) == ST_INVALID_ARG and b"member -1" in msg()
        assert c_list(fn, [M, members[0]], hs) == ST_INVALID_ARG
        assert c_list(fn, [members[0], members[0]], hs) == ST_INVALID_ARG
        assert b"one pending write" in msg() and b"a second time" in msg()
        assert fn(bank._h, None, (C.c_void_p * 2)(*hs), 2, buf.ctypes.data_as(I64P)) == ST_INVALID_ARG
        assert fn(bank._h, (C.c_int * 2)(*members), None, 2, buf.ctypes.data_as(I64P)) == ST_INVALID_ARG
        assert c_list(fn, members, [hs[0], None]) == ST_INVALID_ARG
        assert c_list(fn, members, [hs[0], w.addrs[0]._bank(other)]) == ST_INVALID_ARG and b"does not belong" in msg()
        assert c_list(fn, members, [hs[0], empty._bank(bank)]) == ST_INVALID_ARG and b"empty address" in msg()

    other = w.new_bank(2)
    empty = pkg.Address.alloc(bank)
    snaps = [member_snapshot(bank, m) for m in range(M)]
    argument_refusals(RPW, [2, 0])
    unchanged("read_prepare_write list: arguments")
    # a write list naming a member in state 0 (all of them, then one of two)
    assert c_list(WR, [2, 0], [h[2], h[0]], data=wct) == ST_STATE and b"member 2" in msg()
    unchanged("write list in state 0")
    # keys not loaded; a named member never uploaded
    other_snaps = [member_snapshot(other, m) for m in range(2)]
    assert c_list(RPW, [1, 0], [w.addrs[0]._bank(other), w.addrs[1]._bank(other)], on=other) == ST_KEYS
    assert b"keys" in L.fheram_bank_last_error(other._h)
    for m in range(2):
        assert_member_is(other, m, other_snaps[m], "keys not loaded")
    partial = w.new_bank(3, load=False)
    partial.load_encrypted(0, w.rows[0])
    partial.load_encrypted(1, w.rows[1])
    with pytest.raises(pkg.FheRamError) as e:
        rpw_list(w, partial, [2, 0])
    assert e.value.code == ST_UNINITIALIZED and "member 2" in e.value.msg
    assert partial.state(0) is False and np.array_equal(partial.store_encrypted(0), w.rows[0])
    # the Python layer
    for bad in (lambda: bank.read_prepare_write_list([], [], w.keys), lambda: bank.read_prepare_write_list([0, 2], [w.addrs[0]], w.keys),
                lambda: bank.read_prepare_write_list([0, 2], [w.addrs[0], None], w.keys), lambda: bank.read_prepare_write_list([0, 0], [w.addrs[0]] * 2, w.keys),
                lambda: bank.write_list([0, 2], None, [w.addrs[0]] * 2, w.keys), lambda: bank.write_list([0, 2], wct[:1], [w.addrs[0]] * 2, w.keys)):
        with pytest.raises(pkg.FheRamError) as e:
            bad()
        assert e.value.code == ST_INVALID_ARG
    unchanged("python layer")
    # prepared members: a second read_prepare_write list is refused, and so is every bad write list
    check_prepared(w, bank, [2, 0], rpw_list(w, bank, [2, 0]), "prepare")
    snaps = [member_snapshot(bank, m) for m in range(M)]
    assert c_list(RPW, [1, 2], [h[1], h[2]]) == ST_STATE and b"member 2" in msg()
    assert c_list(WR, [2, 1], [h[2], h[1]], data=wct) == ST_STATE and b"member 1" in msg()
    unchanged("state")
    argument_refusals(WR, [2, 0])
    assert c_list(WR, [2, 0], [h[2], h[0]], data=None) == ST_INVALID_ARG
    unchanged("write list: arguments")
    # a limb out of range: no row is touched, the members stay prepared, and the correct write behind it is the standalone one
    bad_words = np.stack([wct[2], wct[0]]).copy()
    bad_words[1, w.ws - 1, 17] = 1 << 16 | 1
    assert c_list(WR, [2, 0], [h[2], h[0]], data=bad_words) == ST_RANGE
    unchanged("a limb out of range")
    write_list(w, bank, [2, 0])
    check_written(w, bank, [2, 0], "behind the refusals")
    assert_snap(snap(w, bank, 1), (w.rows[1], None, False), "member 1")


@pytest.mark.parametrize("nth", [1, 7, 11], ids=["first-arena", "behind-the-arenas", "last-buffer"])
def test_buffers_that_cannot_be_allocated_2_14(w14, nth):
    """FHERAM_ERR_DEVICE: the nth of the eleven allocations of the lists' buffers fails (fheram_bank_selftest_fail_list_alloc: what an
    exhausted device makes hipMalloc return).  The call changes nothing, the bank holds no half set of buffers, and every other operation
    — ranges, read lists, and the same list again — still works.  Then the same while the buffers GROW under prepared members."""
    w = w14
    pkg = w.pkg
    vals, wct = words_of(w)
    bank = w.new_bank(3)
    last = bank.read_list([0, 1], [w.addrs[0], w.addrs[1]], w.keys).copy()
    snaps = [snap(w, bank, m) for m in range(3)]
    bank.selftest_fail_list_alloc(nth)
    with pytest.raises(pkg.FheRamError) as e:
        rpw_list(w, bank, [2, 0])
    assert e.value.code == ST_DEVICE and "write list" in e.value.msg
    for m in range(3):
        assert_snap(snap(w, bank, m), snaps[m], ("refused for its buffers", m))
    assert np.array_equal(bank.list_result(0, 2), last)
    got = bank.read_prepare_write([w.addrs[J[1]]], w.keys, first=1)       # a range, a read list and the list itself still work
    check_prepared(w, bank, [1], got, "a range behind the refusal")
    assert np.array_equal(bank.read_list([0, 2], [w.addrs[0], w.addrs[1]], w.keys)[1], w.new_bank(3).read([w.addrs[1]], w.keys, first=2)[0])
    check_prepared(w, bank, [2, 0], rpw_list(w, bank, [2, 0]), "the list behind the refusal")
    # growth from two entries to three, with all three members prepared: refused, they stay prepared, and the write behind it is the standalone one
    snaps = [snap(w, bank, m) for m in range(3)]
    bank.selftest_fail_list_alloc(nth)
    with pytest.raises(pkg.FheRamError) as e:
        write_list(w, bank, [1, 2, 0])
    assert e.value.code == ST_DEVICE
    for m in range(3):
        assert_snap(snap(w, bank, m), snaps[m], ("growth refused", m))
    check_prepared(w, bank, [1, 2, 0], None, "growth refused")
    bank.write(wct[1:2], [w.addrs[J[1]]], w.keys, first=1)                 # a range write, then the list of the other two
    write_list(w, bank, [0, 2])
    check_written(w, bank, [0, 1, 2], "behind the refused growth")
