"""fheram_bank_read_prepare_write_mix (RamBank.read_prepare_write_mix): the reads of a step and the first halves of its writes under ONE
top (include/fheram.h).

The contract: the call is np.array_equal, on int64, to the sequence read_mix(reads), read_prepare_write_list(prepare list),
RegFile.read_prepare_write(selector) — in its five outputs and in what it leaves on the bank: rows, tree level 0, states and result slots
of the members, the register file's rotated row, state and kept trace, the read kinds' last outputs.  Every test drives a TWIN bank with
that sequence (same rows, same handles' digits) and compares; the prepared halves are also compared with the oracle's
Ram::read_prepare_write, and the writes that follow with its Ram::write.  Banks have two members at word_size 2 over DECOMP_N = [3,3,3,3],
a 12-bit table and a 5-bit register file (2 digits) unless a test says otherwise; the three shapes are those at which the top changes
form (test_gpu_mix.py): 2^12 no coordinate-1 products, 2^13 one digit (unfused), 2^16 two digits (the tail form).  The worlds and helpers
are test_gpu_mix.py's, test_gpu_regs.py's, test_gpu_table.py's and test_gpu_select.py's."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import lib, sha
from test_gpu_mix import groups, keyed_bank, kit, reads_of, w16, world  # noqa: F401 (w16: fixture)
from test_gpu_regs import enc_digits, oaddr, oram_of, orow, w2, w13  # noqa: F401 (w2, w13: fixtures)
from test_gpu_regs import selector as narrow_selector

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS = 1, 2, 3, 4
RD = 7   # the register rd names (rs1, rs2: the kit's 19 and 4)


def twins(w, config=None, twin_config=None, **kw):
    """(the bank the mix runs on, its twin for the sequence): the same rows, table and register file"""
    return kit(w, keyed_bank(w, config), **kw), kit(w, keyed_bank(w, config if twin_config is None else twin_config), **kw)


def rd_of(k):
    return narrow_selector(k.w, k.bank, RD % (1 << k.rb), k.rb)


def mix(k, reads=(None, None, None), plist=None, rd=None, download=True):
    return k.bank.read_prepare_write_mix(reads[0], reads[1], reads[2], prepare_list=plist, prepare_regs=(k.rf, rd) if rd is not None else None, download=download)


def sequence(k, reads=(None, None, None), plist=None, rd=None, download=True):
    """the three calls the mix promises to equal, in their order"""
    w, out = k.w, [None] * 5
    if any(g is not None for g in reads):
        out[:3] = k.bank.read_mix(*reads, download=download)
    if plist is not None:
        out[3] = k.bank.read_prepare_write_list(plist[0], plist[1], w.keys, download=download)
    if rd is not None:
        out[4] = k.rf.read_prepare_write(rd, download=download)
    return tuple(out)


def assert_outputs(got, want, what):
    for name, g, x in zip(("list", "table", "regs", "prepared list", "prepared regs"), got, want):
        assert (g is None) == (x is None), (what, name)
        if g is not None:
            assert g.shape == x.shape and np.array_equal(g, x), (what, name, np.count_nonzero(g != x))


def snapshot(k, members=(0, 1), results=(), old=False):
    """everything the contract names: rows, states, tree level 0 (two coordinates), the result slots of `results`, the register file"""
    bank, two = k.bank, k.w.max_addr > (1 << 12)
    s = {f"rows {m}": bank.store_encrypted(m) for m in members}
    s.update({f"state {m}": bank.state(m) for m in members})
    if two:
        s.update({f"tree {m}": bank.tree(m, 0) for m in members})
    s.update({f"result {m}": bank.result(m, 1) for m in results})
    s["regs row"], s["regs state"] = k.rf.store(), k.rf.state()
    if old:
        s["regs old"] = k.rf.old_result()
    return s


def assert_snapshots(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


def oracle_member(w, m, j):
    """(the oracle's RAM of member m after read_prepare_write at address j, the old word)"""
    om = w.new_oram(m)
    return om, om.read_prepare_write(w.o.address_new(w.addr_g[j]), w.okeys)


def assert_member_is_oracle(k, m, om, what):
    assert np.array_equal(k.bank.store_encrypted(m), om.store()), (what, "rows")
    if k.w.max_addr > (1 << 12):
        assert np.array_equal(k.bank.tree(m, 0).ravel(), np.asarray(om.tree(0)).ravel()), (what, "tree")


def tail_delta(bank, run):
    a = bank.tail_stats()
    out = run()
    b = bank.tail_stats()
    return b["launches"] - a["launches"], b["fallbacks"] - a["fallbacks"], out


def write_both_halves(ks, cts, plist, rd, S):
    """write_list on the prepared members and the register write, on every bank of ks"""
    for k in ks:
        k.bank.write_list(plist[0], cts[:len(plist[0])], plist[1], k.w.keys)
        if rd:
            k.rf.write(rd_of(k), S.host(2), host_words=cts)


# ---- 1. prepares only ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12, 16])
def test_prepares_only(request, shape):
    """member 0 and the register file: Y = 4.  Against the twin's single calls and against the oracle; then both writes."""
    w = world(request, shape)
    S, a = w.pkg.Src, w.addrs
    km, kt = twins(w)
    plist = ([0], [a[0]])
    launches, fallbacks, got = tail_delta(km.bank, lambda: mix(km, plist=plist, rd=rd_of(km)))
    want = sequence(kt, plist=plist, rd=rd_of(kt))
    assert got[:3] == (None, None, None)
    assert_outputs(got, want, shape)
    assert_snapshots(snapshot(km, results=(0,), old=True), snapshot(kt, results=(0,), old=True), shape)
    assert km.bank.state(0) and not km.bank.state(1) and km.rf.state()
    if shape != 13:   # (2^13: the alone packer levels of 2 rows x 2 ciphertexts are a tail chain of the member's own stage)
        assert (launches, fallbacks) == (1, 0), (shape, launches, fallbacks)
    om, old = oracle_member(w, 0, 0)
    assert np.array_equal(got[3][0], old), "the old word is not the oracle's"
    assert_member_is_oracle(km, 0, om, shape)
    oram, okeys = oram_of(w, km.rb, km.rrow), w.small(km.rb)[1]
    assert np.array_equal(got[4], oram.read_prepare_write(oaddr(w, RD, km.rb), okeys)), "the old register word is not the oracle's"
    assert np.array_equal(km.rf.store(), orow(w, oram)) and np.array_equal(km.rf.old_result(), got[4])
    # the second halves resume as after the single calls
    vals, cts = w.candidates(3, seed=52)
    write_both_halves((km, kt), cts, plist, True, S)
    assert_snapshots(snapshot(km), snapshot(kt), (shape, "after the writes"))
    om.write(cts[0], w.o.address_new(w.addr_g[0]), w.okeys)
    oram.write(cts[2], oaddr(w, RD, km.rb), okeys)
    assert np.array_equal(km.bank.store_encrypted(0), om.store()) and np.array_equal(km.rf.store(), orow(w, oram))
    assert not km.bank.state(0) and not km.rf.state()
    back = km.bank.read([a[0]], w.keys, first=0)
    assert np.array_equal(back, kt.bank.read([a[0]], w.keys, first=0))
    w.check_value(back[0], vals[0], "the written word")


# ---- 2. a full step ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 16])
def test_a_full_step(request, shape):
    """the data read of member 1, the fetch, rs1 and rs2, and the preparations of member 0 and of rd in the SAME register file: Y = 12"""
    w = world(request, shape)
    S, a = w.pkg.Src, w.addrs
    km, kt = twins(w)
    plist = ([0], [a[0]])
    got = mix(km, groups(km, 1, 1, 2), plist, rd_of(km))
    want = sequence(kt, groups(kt, 1, 1, 2), plist, rd_of(kt))
    assert_outputs(got, want, shape)
    assert_snapshots(snapshot(km, results=(0, 1), old=True), snapshot(kt, results=(0, 1), old=True), shape)
    for k, out in ((km, got), (kt, want)):
        assert np.array_equal(k.bank.list_result(0, 1), out[0]) and np.array_equal(k.bank.table_result(0, 1), out[1]) and np.array_equal(k.rf.result(0, 2), out[2])
    assert np.array_equal(got[3][0], oracle_member(w, 0, 0)[1])
    oram, okeys = oram_of(w, km.rb, km.rrow), w.small(km.rb)[1]
    for e in range(2):   # rs1 and rs2 saw the row before rd's products landed in it
        assert np.array_equal(got[2][e], oram.read(oaddr(w, km.r_idx[e], km.rb), okeys)), e
    assert np.array_equal(got[4], oram.read_prepare_write(oaddr(w, RD, km.rb), okeys))
    vals, cts = w.candidates(3, seed=52)
    write_both_halves((km, kt), cts, plist, True, S)
    assert_snapshots(snapshot(km), snapshot(kt), (shape, "after the writes"))


# ---- 3. a member read and prepared in one call ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12])
@pytest.mark.parametrize("config", [None, {"memo": 0}], ids=["default", "memo0"])
def test_a_member_in_both_lists(request, shape, config):
    """member 0 read at address 1 and prepared at address 2 in ONE call: the read is the one taken before any preparation (its packed row
    and its digits survive the preparation, which runs on the same arenas); memo = 0: the member's result slot is the preparation's"""
    w = world(request, shape)
    a = w.addrs
    km, kt = twins(w, config)
    before = km.bank.read([a[1]], w.keys, first=0)
    reads, plist = (([0], [a[1]]), None, None), ([0], [a[2]])
    got = mix(km, reads, plist)
    assert np.array_equal(got[0][0], before[0]), "the read saw the preparation"
    assert_outputs(got, sequence(kt, reads, plist), (shape, config))
    assert_snapshots(snapshot(km, results=(0,)), snapshot(kt, results=(0,)), (shape, config))
    assert np.array_equal(km.bank.result(0, 1)[0], got[3][0]) and np.array_equal(km.bank.list_result(0, 1), got[0])
    om, old = oracle_member(w, 0, 2)
    assert np.array_equal(got[3][0], old)
    assert_member_is_oracle(km, 0, om, (shape, config))


# ---- 4. the dense plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 16])
def test_a_dense_prepare_list_and_a_range_write(request, shape):
    """the prepare list [1, 0] is no range: it runs on the write lists' own set and hands over into the members' slots.  A RANGE write of both
    members resumes from those slots; then the same list again and write_list, which resumes from the set itself"""
    w = world(request, shape)
    a = w.addrs
    km, kt = twins(w)
    vals, cts = w.candidates(3, seed=52)
    plist = ([1, 0], [a[1], a[2]])
    for follow in ("range", "list"):
        got = mix(km, (None, None, (km.rf, km.rsel[:1])), plist)
        assert_outputs(got, sequence(kt, (None, None, (kt.rf, kt.rsel[:1])), plist), (shape, follow))
        assert_snapshots(snapshot(km, results=(0, 1)), snapshot(kt, results=(0, 1)), (shape, follow))
        for k in (km, kt):
            if follow == "range":
                k.bank.write(cts[:2], [a[2], a[1]], w.keys, first=0)   # member 0 at address 2, member 1 at address 1
            else:
                k.bank.write_list(plist[0], cts[1:3], plist[1], w.keys)
        assert_snapshots(snapshot(km), snapshot(kt), (shape, follow, "after the write"))
    om0, _ = oracle_member(w, 0, 2)
    om0.write(cts[0], w.o.address_new(w.addr_g[2]), w.okeys)
    om0.read_prepare_write(w.o.address_new(w.addr_g[2]), w.okeys)
    om0.write(cts[2], w.o.address_new(w.addr_g[2]), w.okeys)
    assert np.array_equal(km.bank.store_encrypted(0), om0.store())


# ---- 5. a single prepare entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12])
def test_a_single_prepare_entry(request, shape):
    """one member and nothing else: followed by write_list, and followed by a single-member write (which computes the inverse digits
    itself: the mix starts none early)"""
    w = world(request, shape)
    a = w.addrs
    km, kt = twins(w)
    vals, cts = w.candidates(3, seed=52)
    plist = ([1], [a[1]])
    om = w.new_oram(1)
    for i, follow in enumerate(("list", "single")):
        got = mix(km, plist=plist)
        assert_outputs(got, sequence(kt, plist=plist), (shape, follow))
        assert_snapshots(snapshot(km, results=(1,)), snapshot(kt, results=(1,)), (shape, follow))
        assert np.array_equal(got[3][0], om.read_prepare_write(w.o.address_new(w.addr_g[1]), w.okeys))
        for k in (km, kt):
            if follow == "list":
                k.bank.write_list(plist[0], cts[i:i + 1], plist[1], w.keys)
            else:
                k.bank.write(cts[i:i + 1], plist[1], w.keys, first=1)
        om.write(cts[i], w.o.address_new(w.addr_g[1]), w.okeys)
        assert_snapshots(snapshot(km), snapshot(kt), (shape, follow, "after the write"))
        assert np.array_equal(km.bank.store_encrypted(1), om.store()), (shape, follow)


# ---- 6. empty read groups ----------------------------------------------------------------------------------------------------------------
def test_empty_read_groups_keep_their_last_outputs(w2):
    """three mixed reads of one kind each leave every kind's outputs in a buffer of the mix; a call with reads = NULL, with empty groups and
    with one kind then keeps what it does not name.  REGS_OLD moves only when the register file is prepared."""
    w, pkg, a = w2, w2.pkg, w2.addrs
    S = pkg.Src
    k = kit(w, keyed_bank(w), tb=6)
    vals, cts = w.candidates(3, seed=52)
    k.rf.read_prepare_write(k.rsel[1], download=False)
    k.rf.write(k.rsel[1], S.regs_old())
    old0 = k.rf.old_result()
    lst = k.bank.read_mix(groups(k, 2, 0, 0)[0], None, None)[0]
    tab = k.bank.read_mix(None, groups(k, 0, 2, 0)[1], None)[1]
    reg = k.bank.read_mix(None, None, groups(k, 0, 0, 2)[2])[2]

    def kept(names):
        for name, want, dl in (("list", lst, lambda: k.bank.list_result(0, 2)), ("table", tab, lambda: k.bank.table_result(0, 2)), ("regs", reg, lambda: k.rf.result(0, 2))):
            if name in names:
                assert np.array_equal(dl(), want), name

    plist = ([0], [a[0]])
    got = mix(k, plist=plist)   # no reads at all: a null struct would do (below), the mirror passes empty groups
    kept(("list", "table", "regs"))
    assert np.array_equal(k.rf.old_result(), old0), "REGS_OLD moved without a prepared register file"
    assert np.array_equal(got[3][0], oracle_member(w, 0, 0)[1])
    k.bank.write_list(plist[0], cts[:1], plist[1], w.keys)
    prep = pkg.api._CMixPrepares()
    members, addrs = (C.c_int * 1)(1), (C.c_void_p * 1)(a[1]._bank(k.bank))
    prep.members, prep.addrs, prep.n_list = members, addrs, 1
    k.bank._chk(lib().fheram_bank_read_prepare_write_mix(k.bank._h, None, C.byref(prep), None, None, None, None, None))   # reads = NULL
    kept(("list", "table", "regs"))
    assert k.bank.state(1) and np.array_equal(k.bank.result(1, 1)[0], oracle_member(w, 1, 1)[1])
    got = mix(k, (None, groups(k, 0, 1, 0)[1], None), rd=rd_of(k))   # the table kind alone, and rd
    kept(("list", "regs"))
    assert np.array_equal(k.bank.table_result(0, 1), got[1]) and np.array_equal(got[1][0], tab[0])
    assert np.array_equal(k.rf.old_result(), got[4]) and not np.array_equal(got[4], old0)
    sel = k.bank.select([narrow_selector(w, k.bank, 1, 1)], [[S.list(1), S.regs(1)]])
    assert np.array_equal(sel[0], w.oselect(1, np.stack([lst[1], reg[1]]), enc_digits(w, 1, 1)))


# ---- 7. a one-digit register file ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12])
def test_a_register_file_of_two_bits(request, shape):
    """2 bits are ONE digit, which the tail's product steps do not take: the unfused form at Y = 6"""
    w = world(request, shape)
    S, a = w.pkg.Src, w.addrs
    km, kt = twins(w, rb=2)
    assert km.rsel[0].n_digits() == 1 and rd_of(km).n_digits() == 1
    plist = ([0], [a[0]])
    reads = (None, None, (km.rf, km.rsel[:1]))
    got = mix(km, reads, plist, rd_of(km))
    assert_outputs(got, sequence(kt, (None, None, (kt.rf, kt.rsel[:1])), plist, rd_of(kt)), shape)
    assert_snapshots(snapshot(km, results=(0,), old=True), snapshot(kt, results=(0,), old=True), shape)
    oram, okeys = oram_of(w, 2, km.rrow), w.small(2)[1]
    assert np.array_equal(got[2][0], oram.read(oaddr(w, km.r_idx[0], 2), okeys))
    assert np.array_equal(got[4], oram.read_prepare_write(oaddr(w, RD % 4, 2), okeys)) and np.array_equal(km.rf.store(), orow(w, oram))
    vals, cts = w.candidates(3, seed=52)
    write_both_halves((km, kt), cts, plist, True, S)
    assert_snapshots(snapshot(km), snapshot(kt), (shape, "after the writes"))


# ---- 8. configurations -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [13, 12])
@pytest.mark.parametrize("config", [{"safe": 1, "monitor": 2}, {"tail": 0, "fuse": 0}, {"tail_ep": 0}, {"memo": 0}], ids=["safe_monitor2", "tail0_fuse0", "tail_ep0", "memo0"])
def test_under_other_configurations(request, shape, config):
    """a read of each kind and both preparations under `safe` with the monitor on every launch, without the tail launch and the fused chains,
    without product steps in the tail and without the kept traces: the sequence's int64 under the same configuration, the oracle's old
    words, no FHERAM_ERR_PRECISION; the writes resume"""
    w = world(request, shape)
    S, a = w.pkg.Src, w.addrs
    km, kt = twins(w, config)
    plist = ([0], [a[0]])
    got = mix(km, groups(km, 1, 1, 1), plist, rd_of(km))
    assert_outputs(got, sequence(kt, groups(kt, 1, 1, 1), plist, rd_of(kt)), (shape, config))
    assert_snapshots(snapshot(km, results=(0, 1), old=True), snapshot(kt, results=(0, 1), old=True), (shape, config))
    om, old = oracle_member(w, 0, 0)
    assert np.array_equal(got[3][0], old)
    assert_member_is_oracle(km, 0, om, (shape, config))
    assert np.array_equal(got[4], oram_of(w, km.rb, km.rrow).read_prepare_write(oaddr(w, RD, km.rb), w.small(km.rb)[1]))
    vals, cts = w.candidates(3, seed=52)
    write_both_halves((km, kt), cts, plist, True, S)
    assert_snapshots(snapshot(km), snapshot(kt), (shape, config, "after the writes"))
    print(f"rpw mix 2^{shape} {config}: round-off maximum {km.bank.roundoff_max():.4f}")   # (raises FHERAM_ERR_PRECISION above 3/8)


# ---- 9. the fallback -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [12, 16])
def test_the_tail_gives_up_and_the_fallback_redoes_it(request, shape):
    """tail_test = 1: the one tail launch of the call gives up late and its predicated fallback redoes every ciphertext.  The twin runs the
    sequence under the DEFAULT configuration.  Rows, trees and the register row are compared.  What this comparison can and cannot tell:
    the hook gives up LATE (two steps before the end of group 0's chain), when the tail launch itself has stored every group's last product,
    so a fallback built WITHOUT store_ep still passes here (tried with such a build: 2^12 and 2^16 both pass) — its stores matter for a
    launch that gives up before its products are done, which the hook cannot stage.  A fallback that stored a WRONG last product, or one
    whose trace did not restart from the sources, fails."""
    w = world(request, shape)
    S, a = w.pkg.Src, w.addrs
    km, kt = twins(w, {"tail_test": 1}, twin_config={})
    plist = ([0], [a[0]])
    reads = lambda k: (None, None, (k.rf, k.rsel[:1]))   # noqa: E731
    launches, fallbacks, got = tail_delta(km.bank, lambda: mix(km, reads(km), plist, rd_of(km)))
    assert launches == 1 and fallbacks >= 1, (shape, launches, fallbacks)
    assert_outputs(got, sequence(kt, reads(kt), plist, rd_of(kt)), shape)
    assert_snapshots(snapshot(km, results=(0,), old=True), snapshot(kt, results=(0,), old=True), shape)
    om, old = oracle_member(w, 0, 0)
    assert np.array_equal(got[3][0], old)
    assert_member_is_oracle(km, 0, om, shape)
    vals, cts = w.candidates(3, seed=52)
    write_both_halves((km, kt), cts, plist, True, S)
    assert_snapshots(snapshot(km), snapshot(kt), (shape, "after the writes"))


# ---- 10. no host wait ------------------------------------------------------------------------------------------------------------------
def test_a_step_without_a_host_wait(w13):
    """every output NULL; a select over [REGS_OLD, HOST] and over [MEMBER_RESULT, HOST]; write_list_selected and the register write of a
    SELECT_RESULT; ONE sync.  Rows and register row equal the sequence's, and the bank's own decrypt gives the expected words: member 0
    takes its old word back, register rd the host word."""
    w, pkg, a = w13, w13.pkg, w13.addrs
    S = pkg.Src
    km, kt = twins(w)
    vals, cts = w.candidates(3, seed=52)
    plist = ([0], [a[0]])

    def step(k, first_halves):
        out = first_halves(k, groups(k, 1, 1, 2), plist, rd_of(k), download=False)
        assert out == (None,) * 5
        picks = [narrow_selector(w, k.bank, 1, 1), narrow_selector(w, k.bank, 0, 1)]
        assert k.bank.select(picks, [[S.regs_old(), S.host(0)], [S.member(0), S.host(1)]], host_words=cts, download=False) is None
        k.bank.write_list_selected([0], [1], plist[1], w.keys)
        k.rf.write(rd_of(k), S.select(0))
        k.bank.sync()

    step(km, mix)
    step(kt, sequence)
    assert_snapshots(snapshot(km), snapshot(kt), "a step without a host wait")
    assert not km.bank.state(0) and not km.rf.state()
    dsk = pkg.GLWESecret(km.bank, w.sk)
    o, kpt = w.o, w.o.p.k_glwe_pt
    values, _ = km.bank.decrypt(0, dsk)
    assert np.array_equal(values, np.array([o.expected_plain(int(x), kpt) for x in w.data[0]]).reshape(-1, w.ws)), "member 0 did not take its old word back"
    regs, _ = km.rf.decrypt(dsk)
    want = np.array([o.expected_plain(int(x), kpt) for x in km.rdata]).reshape(-1, w.ws)
    want[RD] = [o.expected_plain(int(v), kpt, True) for v in vals[0]]
    assert np.array_equal(regs, want), "register rd did not take the host word"


# ---- 11. refusals ----------------------------------------------------------------------------------------------------------------------
def prepares_of(pkg, members, addrs, regs, sel):
    """a fheram_mix_prepares over raw handles"""
    p = pkg.api._CMixPrepares()
    p._keep = [(C.c_int * max(len(members), 1))(*members), (C.c_void_p * max(len(addrs), 1))(*addrs)]
    if members:
        p.members, p.addrs, p.n_list = p._keep[0], p._keep[1], len(members)
    p.regs, p.reg_sel = regs, sel
    return p


def raw(bank, reads, prepares):
    bank._chk(lib().fheram_bank_read_prepare_write_mix(bank._h, C.byref(reads) if reads is not None else None, C.byref(prepares) if prepares is not None else None,
                                                       None, None, None, None, None))


def test_refusals_change_nothing(w13):
    w, pkg, a = w13, w13.pkg, w13.addrs
    S = pkg.Src
    L = lib()
    bank, other, fresh, bare = keyed_bank(w), w.new_bank(1), w.new_bank(2), w.new_bank(2, load=False)   # fresh: keys not loaded; bare: no rows
    other._use_keys(w.keys)
    bare._use_keys(w.keys)
    k = kit(w, bank)
    rd, rf2 = rd_of(k), bank.regfile(5)
    rf2.load(k.rrow)
    first = bank.read_mix(*groups(k, 2, 2, 2))
    bank.read_prepare_write([a[0]], w.keys, first=0)       # member 0 sits in state 1 with a result ...
    k.rf.read_prepare_write(k.rsel[1], download=False)     # ... and so does the kit's register file, with a kept trace; rf2 is in state 0
    ah = [x._bank(bank) for x in a]
    no_reads = pkg.api._CMixReads()

    def digest():
        return ([sha(bank.store_encrypted(m)) for m in range(2)], [bank.state(m) for m in range(2)], [sha(bank.tree(m, 0)) for m in range(2)], sha(bank.result(0, 2)),
                sha(k.rf.store()), k.rf.state(), sha(k.rf.old_result()), sha(rf2.store()), rf2.state(),
                sha(bank.list_result(0, 2)), sha(bank.table_result(0, 2)), sha(k.rf.result(0, 2)))

    def refused(code, call, what):
        before = digest()
        with pytest.raises(pkg.FheRamError) as e:
            call()
        assert e.value.code == code, (what, e.value)
        assert e.value.msg, what
        assert digest() == before, what

    m1 = ([1], [a[1]])
    rf2_rd = narrow_selector(w, bank, RD, 5)
    table_reads = lambda n: reads_of(pkg, [], [], [k.t._h] * n, [k.tsel[0]._h] * n, None, [])   # noqa: E731
    refused(ST_INVALID_ARG, lambda: raw(bank, table_reads(1), prepares_of(pkg, [], [], None, None)), "empty prepares")
    refused(ST_INVALID_ARG, lambda: raw(bank, table_reads(1), None), "null prepares")
    refused(ST_INVALID_ARG, lambda: raw(bank, table_reads(7), prepares_of(pkg, [1], [ah[1]], rf2._h, rf2_rd._h)), "9 entries")
    neg = prepares_of(pkg, [1], [ah[1]], None, None)
    neg.n_list = -1
    refused(ST_INVALID_ARG, lambda: raw(bank, table_reads(1), neg), "a negative count")
    refused(ST_INVALID_ARG, lambda: raw(bank, no_reads, prepares_of(pkg, [1, 1], [ah[1], ah[2]], None, None)), "a member twice in prepares")
    refused(ST_INVALID_ARG, lambda: raw(bank, no_reads, prepares_of(pkg, [1, 0, 1], [ah[1], ah[2], ah[0]], None, None)), "more entries than members")
    refused(ST_STATE, lambda: bank.read_prepare_write_mix(prepare_list=([0], [a[0]])), "a prepared member in state 1")
    refused(ST_STATE, lambda: bank.read_prepare_write_mix(prepare_list=([1, 0], [a[1], a[0]])), "a prepared member in state 1, second in a list")
    refused(ST_STATE, lambda: bank.read_prepare_write_mix(list=([0], [a[0]]), prepare_list=m1), "a read member in state 1")
    refused(ST_STATE, lambda: bank.read_prepare_write_mix(prepare_regs=(k.rf, rd)), "the register file in state 1, as prepares")
    refused(ST_STATE, lambda: bank.read_prepare_write_mix(regs=(k.rf, k.rsel[:1]), prepare_list=m1), "the register file in state 1, as reads")
    refused(ST_INVALID_ARG, lambda: bank.read_prepare_write_mix(prepare_regs=(rf2, k.tsel[0])), "a wide selector on the register file")
    refused(ST_INVALID_ARG, lambda: bank.read_prepare_write_mix(prepare_regs=(rf2, narrow_selector(w, bank, 3, 3))), "a 3-bit selector on a 5-bit register file")
    foreign = pkg.Address(other.params, list(w.addr_g[0]))   # (the mirror binds an Address to the bank it is used on: the foreign handle goes in raw)
    refused(ST_INVALID_ARG, lambda: raw(bank, no_reads, prepares_of(pkg, [1], [foreign._bank(other)], None, None)), "a foreign address")
    refused(ST_INVALID_ARG, lambda: bank.read_prepare_write_mix(prepare_regs=(rf2, narrow_selector(w, other, RD, 5))), "a foreign selector")
    orf = other.regfile(5)
    orf.load(k.rrow)
    refused(ST_INVALID_ARG, lambda: bank.read_prepare_write_mix(prepare_regs=(orf, rf2_rd)), "a foreign register file")
    refused(ST_INVALID_ARG, lambda: raw(bank, no_reads, prepares_of(pkg, [2], [ah[1]], None, None)), "a member outside the bank")
    nul = prepares_of(pkg, [1], [ah[1]], None, None)
    nul.addrs = None
    refused(ST_INVALID_ARG, lambda: raw(bank, no_reads, nul), "a null address list")
    refused(ST_INVALID_ARG, lambda: raw(bank, no_reads, prepares_of(pkg, [], [], rf2._h, None)), "a null selector")
    assert L.fheram_bank_read_prepare_write_mix(None, None, C.byref(prepares_of(pkg, [1], [ah[1]], None, None)), None, None, None, None, None) == ST_INVALID_ARG
    # keys not loaded; a member without rows
    with pytest.raises(pkg.FheRamError) as e:
        raw(fresh, None, prepares_of(pkg, [1], [a[1]._bank(fresh)], None, None))
    assert e.value.code == ST_KEYS and not fresh.state(1), e.value
    with pytest.raises(pkg.FheRamError) as e:
        bare.read_prepare_write_mix(prepare_list=([1], [pkg.Address(bare.params, list(w.addr_g[1]))]))
    assert e.value.code == ST_UNINITIALIZED and not bare.state(1), e.value
    # entries * word_size > 64: five entries of a bank of word_size 16 (refused before any group is looked at)
    big = pkg.RamBank(pkg.Parameters(max_addr=1 << 12, word_size=16), 2, 0)
    bt, bs, brf = big.table(6), big.table_selector(6), big.regfile(5)
    with pytest.raises(pkg.FheRamError) as e:
        big.read_prepare_write_mix(tables=([bt] * 4, [bs] * 4), prepare_regs=(brf, big.selector(5)))
    assert e.value.code == ST_INVALID_ARG and "exceeds 64" in e.value.msg, e.value
    # a valid call behind the refusals: member 1 and the free register file, then everything is written
    got = bank.read_prepare_write_mix(prepare_list=m1, prepare_regs=(rf2, rf2_rd))
    assert np.array_equal(got[3][0], oracle_member(w, 1, 1)[1]) and bank.state(1) and rf2.state()
    assert np.array_equal(bank.list_result(0, 2), first[0])
