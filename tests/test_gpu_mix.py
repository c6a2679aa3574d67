"""fheram_bank_read_mix (RamBank.read_mix): a read list, a table read and a register read of one bank as ONE operation with one top
(include/fheram.h).

The contract: entry k of a group is np.array_equal, on int64, to output k of that group's single call on the same bank with the same
handles (reads change no row), and the bank is left where the sequence read_list, table_read, RegFile.read leaves it.  One case per shape
is also compared with the oracle's Ram::read.  Banks have two members at word_size 2 over DECOMP_N = [3,3,3,3]:
  2^12  one row, one coordinate: a list entry has 0 product steps in the top; with a 12-bit table (4 digits) and a 5-bit register file
        (2 digits) the counts are 0 / 4 / 2, all in ONE launch of k_trace_tail_x
  2^13  two rows; get_base_2d gives the second coordinate ONE digit ([[3,3,3,3],[1]]), which the tail's product steps do not take, so the
        counts 1 / 4 / 2 run the products entry by entry and one trace over all six ciphertexts
  2^16  sixteen rows, the second coordinate [3,1]: 2 / 4 / 2, a list entry WITH products inside k_trace_tail_x
The worlds and helpers are test_gpu_regs.py's and test_gpu_table.py's.

Launch counts (fheram_bank_profile_enable, class keyswitch_tail_launch).  The top of a mix is one tail launch and the tops of the three
single calls are three.  The list group's own stage adds L launches to both, where L is what a read list alone takes beyond its top: 0 at
2^12 and 2^16, 1 at 2^13 (the eleven alone packer levels of 2 rows x 2 ciphertexts run as a tail chain themselves).  So the mix counts
1 + L and the sequence 3 + L: exactly 1 and 3 where L = 0, and L is measured on a read list alone where it is not."""
import ctypes as C
import types

import numpy as np
import pytest

from test_gpu_bank import lib, sha
from test_gpu_regs import (decrypts_to, enc_digits, oaddr, oram_of, orow, regs_rows, w2, w13, word_of)  # noqa: F401 (w2, w13: fixtures)
from test_gpu_regs import selector as narrow_selector
from test_gpu_select import SelWorld
from test_gpu_table import loaded_table, oracle_reads, wide

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS = 1, 2, 3, 4
_BANKS = {}


@pytest.fixture(scope="module")
def w16(po):
    return SelWorld(po, 1 << 16, 2, 2, seed=420)


def world(request, shape):
    return request.getfixturevalue({12: "w2", 13: "w13", 16: "w16"}[shape])


def keyed_bank(w, config=None):
    bank = w.new_bank(2, config=config)
    bank._use_keys(w.keys)
    return bank


def shared_bank(w):
    """one default bank per world for the tests that change no row"""
    if id(w) not in _BANKS:
        _BANKS[id(w)] = keyed_bank(w)
    return _BANKS[id(w)]


def kit(w, bank, tb=12, rb=5, t_idx=(3001, 77), r_idx=(19, 4), members=(1, 0), addrs=(1, 2)):
    """a table of tb bits and a register file of rb bits on `bank`, with two entries of each kind: handles, and what they should read"""
    t_idx, r_idx = [i % (1 << tb) for i in t_idx], [i % (1 << rb) for i in r_idx]
    t, tdata, trow = loaded_table(w, bank, tb)
    rdata, rrow = regs_rows(w, rb, seed=1)
    rf = bank.regfile(rb)
    rf.load(rrow)
    return types.SimpleNamespace(w=w, bank=bank, t=t, trow=trow, tdata=tdata, tb=tb, rf=rf, rrow=rrow, rdata=rdata, rb=rb, t_idx=t_idx, r_idx=r_idx,
                                 tsel=[wide(w, bank, i, tb) for i in t_idx], rsel=[narrow_selector(w, bank, i, rb) for i in r_idx],
                                 members=list(members), addr_j=list(addrs), addrs=[w.addrs[j] for j in addrs])


def groups(k, nl, nt, nr, twice=False):
    """the first nl / nt / nr entries of the kit as read_mix's arguments; twice: entry 1 of every group repeats entry 0's member, table and selector"""
    pick = (lambda xs, n: [xs[0]] * n) if twice else (lambda xs, n: xs[:n])
    lst = (pick(k.members, nl), k.addrs[:nl]) if nl else None
    tabs = ([k.t] * nt, pick(k.tsel, nt)) if nt else None
    regs = (k.rf, pick(k.rsel, nr)) if nr else None
    return lst, tabs, regs


def singles(k, lst, tabs, regs, download=True):
    """the three single calls, in the order whose end state the mix promises"""
    w, bank = k.w, k.bank
    return (bank.read_list(lst[0], lst[1], w.keys, download=download) if lst else None,
            bank.table_read(tabs[0], tabs[1], download=download) if tabs else None,
            regs[0].read(regs[1], download=download) if regs else None)


def assert_same(got, want, what):
    for name, g, x in zip(("list", "table", "regs"), got, want):
        assert (g is None) == (x is None), (what, name)
        if g is not None:
            assert g.shape == x.shape and np.array_equal(g, x), (what, name, np.count_nonzero(g != x))


def results(k, lst, tabs, regs):
    """what the three _result downloads give for the groups named"""
    return (k.bank.list_result(0, len(lst[0])) if lst else None, k.bank.table_result(0, len(tabs[0])) if tabs else None,
            k.rf.result(0, len(regs[1])) if regs else None)


def assert_oracle(k, got, nl, nt, nr, twice=False):
    w = k.w
    for e in range(nl):
        m, j = k.members[0 if twice else e], k.addr_j[e]
        want = w.new_oram(m).read(w.o.address_new(w.addr_g[j]), w.okeys)
        assert np.array_equal(got[0][e], want), ("list", e, np.count_nonzero(got[0][e] != want))
        print(f"mix list entry {e}: log2 noise {decrypts_to(w, got[0][e], [int(w.data[m][i + w.ws * w.idx[j]]) for i in range(w.ws)], False):.2f}")
    t_idx = [k.t_idx[0 if twice else e] for e in range(nt)]
    for e, want in enumerate(oracle_reads(w, k.tb, k.trow, t_idx)):
        assert np.array_equal(got[1][e], want), ("table", e)
        print(f"mix table entry {e}: log2 noise {decrypts_to(w, got[1][e], word_of(w, k.tdata, t_idx[e]), False):.2f}")
    oram, okeys = oram_of(w, k.rb, k.rrow), w.small(k.rb)[1]
    for e in range(nr):
        idx = k.r_idx[0 if twice else e]
        assert np.array_equal(got[2][e], oram.read(oaddr(w, idx, k.rb), okeys)), ("regs", e)
        print(f"mix regs entry {e}: log2 noise {decrypts_to(w, got[2][e], word_of(w, k.rdata, idx), False):.2f}")


def tail_launches(bank, run):
    bank.profile_enable(True)
    bank.profile_reset()
    out = run()
    bank.sync()
    n = bank.profile_get("keyswitch_tail_launch")["launches"]
    bank.profile_enable(False)
    return n, out


# ---- 1. one entry of each kind: Y = 6 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12, 16])
def test_one_entry_of_each_kind(request, shape):
    """digit counts 1 / 4 / 2 (2^13), 0 / 4 / 2 (2^12) and 2 / 4 / 2 (2^16): equal to the single calls and to the oracle; one tail launch for the
    top where the single calls take three (module docstring: how the list group's own stage is accounted for)"""
    w = world(request, shape)
    k = kit(w, shared_bank(w))
    assert w.po.get_base_2d(w.max_addr, [3, 3, 3, 3])[1:] == {12: [], 13: [[1]], 16: [[3, 1]]}[shape]
    assert (k.tsel[0].n_digits(), k.rsel[0].n_digits()) == (4, 2)
    lst, tabs, regs = groups(k, 1, 1, 1)
    n_list, _ = tail_launches(k.bank, lambda: k.bank.read_list(lst[0], lst[1], w.keys))
    n_seq, want = tail_launches(k.bank, lambda: singles(k, lst, tabs, regs))
    n_mix, got = tail_launches(k.bank, lambda: k.bank.read_mix(lst, tabs, regs))
    assert_same(got, want, shape)
    assert_same(results(k, lst, tabs, regs), want, (shape, "the _result downloads"))
    assert_oracle(k, got, 1, 1, 1)
    local = n_list - 1   # the list group's own stage
    print(f"2^{shape}: keyswitch_tail_launch {n_mix} for the mix, {n_seq} for the three single calls, {n_list} for the read list alone")
    assert local == (1 if shape == 13 else 0), (shape, n_list)
    assert (n_mix, n_seq) == (1 + local, 3 + local), (shape, n_mix, n_seq, n_list)
    if shape != 13:
        assert (n_mix, n_seq) == (1, 3)
    assert sha(k.t.download()) == sha(k.trow) and sha(k.rf.store()) == sha(k.rrow) and not k.rf.state() and not k.bank.state(1)
    assert np.array_equal(k.bank.result(1, 1)[0], got[0][0]), "member 1 holds the list entry's result, as after its own read"


# ---- 2. groups left out -------------------------------------------------------------------------------------------------------------------------
def test_empty_groups_keep_their_last_outputs(w2):
    """a 6-bit table (2 digits) beside the 5-bit register file at 2^12: list + table (0 / 2), table + regs (2 / 2) and regs alone, each equal to
    its single calls; the kinds left out stay readable — through the _result downloads and as select candidates — whichever buffer held them"""
    w, S = w2, w2.pkg.Src
    k = kit(w, shared_bank(w), tb=6)
    assert k.tsel[0].n_digits() == 2
    first = k.bank.read_mix(*groups(k, 2, 2, 2))
    picks = [narrow_selector(w, k.bank, i, 2) for i in range(3)]

    last = (lambda: k.bank.list_result(0, 2), lambda: k.bank.table_result(0, 2), lambda: k.rf.result(0, 2))   # of the two-entry mix, per kind

    def digest(lst, tabs, regs):
        kept = [None if g else sha(r()) for g, r in zip((lst, tabs, regs), last)]
        cands = [S.zero() if lst else S.list(1), S.zero() if tabs else S.table(1), S.zero() if regs else S.regs(1)]
        return kept, sha(k.bank.select(picks, [cands] * 3))

    for nl, nt, nr in ((1, 1, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 2, 0)):
        lst, tabs, regs = groups(k, nl, nt, nr)
        k.bank.read_mix(*groups(k, 2, 2, 2), download=False)
        before = digest(lst, tabs, regs)
        got = k.bank.read_mix(lst, tabs, regs)
        assert digest(lst, tabs, regs) == before, ((nl, nt, nr), "a group left out lost its last outputs")
        for g, r, f in zip((lst, tabs, regs), last, first):
            if not g:
                assert np.array_equal(r(), f), (nl, nt, nr)
        assert_same(results(k, lst, tabs, regs), got, ((nl, nt, nr), "the _result downloads"))
        assert_same(got, singles(k, lst, tabs, regs), (nl, nt, nr))
    # three mixes in a row, each leaving two kinds out: every kind's outputs survive in a buffer of their own
    a = k.bank.read_mix(groups(k, 2, 0, 0)[0], None, None)[0]
    b = k.bank.read_mix(None, groups(k, 0, 2, 0)[1], None)[1]
    c = k.bank.read_mix(None, None, groups(k, 0, 0, 2)[2])[2]
    d = k.bank.read_mix(groups(k, 1, 0, 0)[0], None, None)[0]
    assert np.array_equal(k.bank.table_result(0, 2), b) and np.array_equal(k.rf.result(0, 2), c) and np.array_equal(k.bank.list_result(0, 1), d)
    assert np.array_equal(a[0], d[0])
    assert_oracle(k, (a, b, c), 2, 2, 2)


# ---- 3. the unfused form --------------------------------------------------------------------------------------------------------------------------
def test_two_entries_of_each_kind(w13):
    """Y = 12 at 2^13: the products entry by entry and one trace over twelve ciphertexts; member 1, the table and one selector of each group
    named twice"""
    w = w13
    k = kit(w, shared_bank(w))
    lst, tabs, regs = groups(k, 2, 2, 2, twice=True)
    assert lst[0] == [1, 1] and tabs[1][0] is tabs[1][1] and regs[1][0] is regs[1][1]
    want = singles(k, lst, tabs, regs)
    got = k.bank.read_mix(lst, tabs, regs)
    assert_same(got, want, "twice")
    assert np.array_equal(got[1][0], got[1][1]) and np.array_equal(got[2][0], got[2][1])
    assert_oracle(k, got, 2, 2, 2, twice=True)
    assert np.array_equal(k.bank.result(1, 1)[0], got[0][1]), "member 1 holds the result of the LAST entry that named it"
    # distinct entries, eight of them: the bound of a call
    lst, tabs, regs = groups(k, 2, 2, 2)
    four = (k.rf, regs[1] + regs[1])
    assert_same(k.bank.read_mix(lst, tabs, four), singles(k, lst, tabs, four), "eight entries")


def test_a_one_digit_register_file(w2, w13):
    """3 bits are one digit, which the tail's product steps do not take: the unfused form at Y <= 8"""
    for w in (w2, w13):
        k = kit(w, shared_bank(w), rb=3)
        assert k.rsel[0].n_digits() == 1
        for nl, nt, nr in ((1, 1, 1), (1, 0, 2), (0, 0, 1)):
            lst, tabs, regs = groups(k, nl, nt, nr)
            got = k.bank.read_mix(lst, tabs, regs)
            assert_same(got, singles(k, lst, tabs, regs), (w.max_addr, nl, nt, nr))
        assert_oracle(k, got, 0, 0, 1)


# ---- 4. configurations ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12])
@pytest.mark.parametrize("config", [{"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}, {"tail_ep": 0}], ids=["safe_monitor2", "tail0_fuse0", "tail_ep0"])
def test_under_other_configurations(request, shape, config):
    """one entry of each kind under `safe` with the monitor on every launch, without the tail launch and the fused chains, and without product
    steps in the tail: the same int64 as the default bank, no FHERAM_ERR_PRECISION"""
    w = world(request, shape)
    kd = kit(w, shared_bank(w))
    default = kd.bank.read_mix(*groups(kd, 1, 1, 1))
    k = kit(w, keyed_bank(w, config))
    lst, tabs, regs = groups(k, 1, 1, 1)
    got = k.bank.read_mix(lst, tabs, regs)
    assert_same(got, default, (shape, config))
    assert_same(got, singles(k, lst, tabs, regs), (shape, config, "the single calls under the same configuration"))
    print(f"mix 2^{shape} {config}: round-off maximum {k.bank.roundoff_max():.4f}")   # (raises FHERAM_ERR_PRECISION above 3/8)


# ---- 5. the fallback ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12, 16])
def test_the_tail_gives_up_and_the_fallback_redoes_it(request, shape):
    """tail_test = 1: member 5 of group 0 gives up two steps before the end of ITS chain (the designed give-up, counted on group 0's own product
    count) and every tail launch of the bank falls back.  The same int64.  fheram_bank_tail_stats, for the top of the mix: one launch; one
    fallback where every ciphertext has products (k_read_chain_x redoes them all: 2^16) or none takes part in the tail's products (2^13, the
    trace-only tail and k_keyswitch_chain), two at 2^12, where the ciphertexts with products and the list group's without take one
    predicated launch each.  At 2^13 the list group's alone levels are a tail chain too: one more launch and fallback, as in a read list alone."""
    w = world(request, shape)
    kd = kit(w, shared_bank(w))
    default = kd.bank.read_mix(*groups(kd, 1, 1, 1))
    k = kit(w, keyed_bank(w, {"tail_test": 1}))
    lst, tabs, regs = groups(k, 1, 1, 1)

    def delta(run):
        a = k.bank.tail_stats()
        out = run()
        b = k.bank.tail_stats()
        return b["launches"] - a["launches"], b["fallbacks"] - a["fallbacks"], out

    l_list, f_list, _ = delta(lambda: k.bank.read_list(lst[0], lst[1], w.keys))
    l_mix, f_mix, got = delta(lambda: k.bank.read_mix(lst, tabs, regs))
    assert_same(got, default, (shape, "tail_test"))
    print(f"2^{shape} tail_test: the mix {l_mix} tail launches, {f_mix} fallbacks; a read list alone {l_list}, {f_list}")
    local = 1 if shape == 13 else 0
    assert (l_list, f_list) == (1 + local, 1 + local), (shape, l_list, f_list)
    assert l_mix == 1 + local, (shape, l_mix)
    assert f_mix - local == (2 if shape == 12 else 1), (shape, f_mix)


# ---- 6. no host wait ------------------------------------------------------------------------------------------------------------------------------
def test_outputs_feed_a_select_and_a_register_write_without_a_host_wait(w2):
    """a mix with every output NULL, then straight away a select over [LIST_RESULT 0, TABLE_RESULT 0, REGS_RESULT 1] and a register write of
    TABLE_RESULT 0: the same as behind the three single calls (Y = 8: the tail form with eight groups)"""
    w, S = w2, w2.pkg.Src
    k = kit(w, keyed_bank(w))
    lst, tabs, regs = groups(k, 1, 1, 2)
    wsel, picks = k.rsel[0], [narrow_selector(w, k.bank, i, 2) for i in range(3)]
    srcs = [S.list(0), S.table(0), S.regs(1)]

    def behind(reads):
        k.rf.load(k.rrow)
        assert reads() in (None, (None, None, None))
        picked = k.bank.select(picks, [srcs] * 3, download=False)
        assert picked is None
        k.rf.read_prepare_write(wsel, download=False)
        k.rf.write(wsel, S.table(0))
        return k.bank.select_result(0, 3), k.rf.store()

    want_sel, want_row = behind(lambda: singles(k, lst, tabs, regs, download=False))
    tres = k.bank.table_result(0, 1)
    got_sel, got_row = behind(lambda: k.bank.read_mix(lst, tabs, regs, download=False))
    assert np.array_equal(got_sel, want_sel), np.count_nonzero(got_sel != want_sel)
    assert np.array_equal(got_row, want_row), np.count_nonzero(got_row != want_row)
    cands = np.stack([k.bank.list_result(0, 1)[0], tres[0], k.rf.result(1, 1)[0]])
    for i in range(3):
        assert np.array_equal(got_sel[i], w.oselect(2, cands, enc_digits(w, i, 2))), i
    oram, okeys = oram_of(w, k.rb, k.rrow), w.small(k.rb)[1]
    oram.read_prepare_write(oaddr(w, k.r_idx[0], k.rb), okeys)
    oram.write(tres[0], oaddr(w, k.r_idx[0], k.rb), okeys)
    assert np.array_equal(got_row, orow(w, oram))


# ---- 7. between two halves --------------------------------------------------------------------------------------------------------------------------
def test_a_mix_inside_a_members_and_a_register_files_write(w13):
    """member 0 sits between read_prepare_write and write and the register file between its own two halves while a mix reads member 1 and the
    table: nothing of the bank moves, and both writes then give the oracle's rows"""
    w, S = w13, w13.pkg.Src
    bank = keyed_bank(w)
    k = kit(w, bank)
    a = w.addrs
    vals, cts = w.candidates(3, seed=52)
    lst0 = bank.read_list([1, 0], [a[1], a[2]], w.keys)
    regs0 = k.rf.read(k.rsel)
    tab0 = bank.table_read([k.t], [k.tsel[1]])
    picked = bank.select([narrow_selector(w, bank, 1, 1)], [[S.host(0), S.list(0)]], host_words=cts)
    bank.read_prepare_write([a[0]], w.keys, first=0)
    k.rf.read_prepare_write(k.rsel[0], download=False)

    def digest():
        return (sha(bank.select_result(0, 1)), sha(k.rf.result(0, 2)), sha(k.rf.old_result()), sha(bank.result(0, 1)), sha(bank.store_encrypted(0)),
                sha(bank.store_encrypted(1)), sha(bank.tree(0, 0)), sha(k.rf.store()), sha(k.t.download()), bank.state(0), bank.state(1), k.rf.state())

    before = digest()
    lst, tabs = ([1], [a[1]]), ([k.t], [k.tsel[0]])
    got = bank.read_mix(lst, tabs, None, download=False)
    assert got == (None, None, None)
    assert digest() == before, "a mix moved something of the bank"
    assert np.array_equal(bank.list_result(0, 1)[0], lst0[0]) and np.array_equal(bank.table_result(0, 1)[0], oracle_reads(w, k.tb, k.trow, k.t_idx[:1])[0])
    assert np.array_equal(k.rf.result(0, 2), regs0) and np.array_equal(bank.select_result(0, 1), picked) and not np.array_equal(bank.table_result(0, 1), tab0)
    with pytest.raises(w.pkg.FheRamError) as e:
        bank.read_mix(lst, tabs, (k.rf, k.rsel[:1]))   # the register file is between its halves: its group is refused as its single call is
    assert e.value.code == ST_STATE and digest() == before, e.value
    with pytest.raises(w.pkg.FheRamError) as e:
        bank.read_mix(([0], [a[0]]), tabs, None)   # ... and so is member 0
    assert e.value.code == ST_STATE and digest() == before, e.value
    k.rf.write(k.rsel[0], S.host(2), host_words=cts)
    oram, okeys = oram_of(w, k.rb, k.rrow), w.small(k.rb)[1]
    oram.read_prepare_write(oaddr(w, k.r_idx[0], k.rb), okeys)
    oram.write(cts[2], oaddr(w, k.r_idx[0], k.rb), okeys)
    assert np.array_equal(k.rf.store(), orow(w, oram)) and not k.rf.state()
    om = w.new_oram(0)
    om.read_prepare_write(w.o.address_new(w.addr_g[0]), w.okeys)
    om.write(cts[1], w.o.address_new(w.addr_g[0]), w.okeys)
    bank.write(cts[1:2], [a[0]], w.keys, first=0)
    assert np.array_equal(bank.store_encrypted(0), om.store()), np.count_nonzero(bank.store_encrypted(0) != om.store())
    assert not bank.state(0)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(w2):
    w, pkg = w2, w2.pkg
    L = lib()
    bank, other, fresh = keyed_bank(w), w.new_bank(1), w.new_bank(2)   # fresh: keys not loaded
    other._use_keys(w.keys)
    k = kit(w, bank)
    t9, _, _ = loaded_table(w, bank, 9)
    t_empty = bank.table(12)
    s9, s5wide = wide(w, bank, 300, 9), wide(w, bank, 19, 5)
    foreign = pkg.Address(other.params, list(w.addr_g[0]))   # (the mirror binds an Address to the bank it is used on: the foreign handle goes in raw)
    lst, tabs, regs = groups(k, 2, 2, 2)
    first = bank.read_mix(lst, tabs, regs)

    def digest():
        return ([sha(bank.store_encrypted(m)) for m in range(2)], [bank.state(m) for m in range(2)], sha(bank.result(0, 2)), sha(k.rf.store()), k.rf.state(),
                sha(k.t.download()), sha(t9.download()), sha(bank.list_result(0, 2)), sha(bank.table_result(0, 2)), sha(k.rf.result(0, 2)))

    def refused(code, call, what):
        before = digest()
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg, what
        assert digest() == before, what

    one = groups(k, 1, 1, 1)
    refused(ST_INVALID_ARG, lambda: bank.read_mix(one[0], one[1], (k.rf, [k.tsel[0]])), "a wide selector in the regs group")
    refused(ST_INVALID_ARG, lambda: bank.read_mix(one[0], ([k.t], [k.rsel[0]]), one[2]), "a 5-bit selector in the table group")
    refused(ST_INVALID_ARG, lambda: bank.read_mix(one[0], ([k.t], [s5wide]), one[2]), "a 5-bit selector made by the wide call in the table group")
    refused(ST_INVALID_ARG, lambda: bank.read_mix(one[0], ([k.t, t9], [k.tsel[0], s9]), one[2]), "tables of 12 and 9 bits together")
    refused(ST_INVALID_ARG, lambda: raw(bank, reads_of(pkg, [1], [foreign._bank(other)], [k.t._h], [k.tsel[0]._h], None, [])), "a foreign bank's address")
    refused(ST_UNINITIALIZED, lambda: bank.read_mix(one[0], ([k.t, t_empty], [k.tsel[0], k.tsel[1]]), one[2]), "an unloaded table")
    refused(ST_INVALID_ARG, lambda: bank.read_mix(([2], [w.addrs[0]]), one[1], one[2]), "a member outside the bank")
    refused(ST_INVALID_ARG, lambda: bank.read_mix(one[0], one[1], (k.rf, [wide(w, other, 3, 5)])), "a selector of another bank")
    kf = kit(w, fresh)
    with pytest.raises(pkg.FheRamError) as e:
        raw(fresh, reads_of(pkg, [], [], [kf.t._h], [kf.tsel[0]._h], None, []))
    assert e.value.code == ST_KEYS, e.value
    # the totals, and the call's own arguments
    reads = reads_of(pkg, [], [], [k.t._h], [k.tsel[0]._h], None, [])
    before = digest()
    assert L.fheram_bank_read_mix(bank._h, None, None, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_read_mix(None, C.byref(reads), None, None, None) == ST_INVALID_ARG
    assert L.fheram_bank_read_mix(bank._h, C.byref(pkg.api._CMixReads()), None, None, None) == ST_INVALID_ARG, "all three groups empty"
    nine = reads_of(pkg, [], [], [k.t._h] * 5, [k.tsel[0]._h] * 5, k.rf._h, [k.rsel[0]._h] * 4)
    assert L.fheram_bank_read_mix(bank._h, C.byref(nine), None, None, None) == ST_INVALID_ARG and b"FHERAM_MIX_MAX" in L.fheram_bank_last_error(bank._h)
    neg = reads_of(pkg, [], [], [k.t._h], [k.tsel[0]._h], None, [])
    neg.n_regs = -1
    assert L.fheram_bank_read_mix(bank._h, C.byref(neg), None, None, None) == ST_INVALID_ARG
    nul = reads_of(pkg, [], [], [k.t._h], [k.tsel[0]._h], None, [])
    nul.table_sels = None
    assert L.fheram_bank_read_mix(bank._h, C.byref(nul), None, None, None) == ST_INVALID_ARG
    assert digest() == before
    # (n_list + n_table + n_regs) * word_size > 64: five entries of a bank of word_size 16 (refused before any group is looked at)
    big = pkg.RamBank(pkg.Parameters(max_addr=1 << 12, word_size=16), 2, 0)
    bt, bs = big.table(6), big.table_selector(6)
    with pytest.raises(pkg.FheRamError) as e:
        big.read_mix(None, ([bt] * 5, [bs] * 5), None)
    assert e.value.code == ST_INVALID_ARG and "exceeds 64" in e.value.msg, e.value
    # a valid mix behind the refusals
    assert_same(bank.read_mix(lst, tabs, regs), first, "behind the refusals")


def raw(bank, reads):
    """fheram_bank_read_mix on a struct of raw handles, without a download"""
    bank._chk(lib().fheram_bank_read_mix(bank._h, C.byref(reads), None, None, None))


def reads_of(pkg, members, addrs, tables, tsels, regs, rsels):
    """a fheram_mix_reads over raw handles (the refusals the Python mirror would make itself)"""
    r = pkg.api._CMixReads()
    r._keep = [(C.c_int * max(len(members), 1))(*members), (C.c_void_p * max(len(addrs), 1))(*addrs), (C.c_void_p * max(len(tables), 1))(*tables),
               (C.c_void_p * max(len(tsels), 1))(*tsels), (C.c_void_p * max(len(rsels), 1))(*rsels)]
    if members:
        r.members, r.addrs, r.n_list = r._keep[0], r._keep[1], len(members)
    if tables:
        r.tables, r.table_sels, r.n_table = r._keep[2], r._keep[3], len(tables)
    if rsels:
        r.regs, r.reg_sels, r.n_regs = regs, r._keep[4], len(rsels)
    return r
