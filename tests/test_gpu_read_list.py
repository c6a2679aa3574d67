"""fheram_bank_read_list / RamBank.read_list: K reads of ANY members of a bank — any order, any repetition, any subset — as ONE
operation (include/fheram.h).

The contract: slice k of a list is int64-identical to the single-member read `bank.read([addrs[k]], keys, first=members[k])` on the
same state (and so, by the bank's own contract, to a standalone Ram and to the oracle); afterwards the bank is where the sequence of
those single-member reads leaves it; members that are not named are untouched, a member between read_prepare_write and write
included; a refused call changes nothing.  No tolerance anywhere: every comparison is np.array_equal on int64."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_bank import CLASSES, World, assert_member_equals_ram, assert_member_is, lib, member_snapshot, profiled

pytestmark = pytest.mark.gpu

ST_INVALID_ARG, ST_STATE, ST_UNINITIALIZED, ST_KEYS = 1, 2, 3, 4
I64P = C.POINTER(C.c_int64)


class Ref:
    """A second, identically loaded bank that only ever runs single-member reads: read (m, j) — member m at address j — is computed once
    and shared, and since a read changes neither rows nor tree, the bank is at any time where ANY sequence of such reads leaves it."""

    def __init__(self, w, M, config=None):
        self.w, self.M = w, M
        self.bank = w.new_bank(M, config=config)
        self._reads = {}

    def read(self, m, j):
        if (m, j) not in self._reads:
            self._reads[(m, j)] = self.bank.read([self.w.addrs[j]], self.w.keys, first=m)[0].copy()
        return self._reads[(m, j)]


def check_list(w, ref, bank, members, js, got):
    """every slice against the single read, then what the list left of every member against what the single reads leave"""
    assert got.shape == (len(members), w.ws, w.params.glwe_len())
    for k, (m, j) in enumerate(zip(members, js)):
        want = ref.read(m, j)
        assert np.array_equal(got[k], want), (members, js, k, np.count_nonzero(got[k] != want))
    for m in range(ref.M):
        assert_member_is(bank, m, member_snapshot(ref.bank, m), (members, "after the list"))
        if m in members:
            last = max(k for k, mk in enumerate(members) if mk == m)
            assert np.array_equal(bank.result(m, 1)[0], got[last]), (members, m)


def run_list(w, bank, members, js, **kw):
    return bank.read_list(members, [w.addrs[j] for j in js], w.keys, **kw)


@pytest.fixture(scope="module")
def w14(po):
    return World(po, 1 << 14, 3, n_addr=4)


@pytest.fixture(scope="module")
def ref14(w14):
    return Ref(w14, 3)


@pytest.fixture(scope="module")
def w16(po):
    """2^16: 16 rows, coordinate 1 has two digits: k_trace_tail_t at n * ws <= 8, the mid chain above it, the fused row chain"""
    return World(po, 1 << 16, 2, seed=80, n_addr=3)


@pytest.fixture(scope="module")
def ref16(w16):
    return Ref(w16, 2)


# ---- 1. equality -----------------------------------------------------------------------------------------------------------------------
# (members, address index per entry); a repeated member gets distinct addresses and, in a case of its own, the same address
LISTS = [([0], [1]), ([0, 0], [0, 1]), ([0, 0], [2, 2]), ([0, 1], [0, 1]), ([1, 0], [0, 1]), ([2, 0], [3, 0]), ([1, 1, 0], [0, 1, 2]),
         ([1, 1, 0], [3, 3, 3]), ([0, 0, 1, 2], [0, 1, 2, 3]), ([2, 1, 0, 2, 1, 0, 2, 1], [0, 1, 2, 3, 0, 1, 2, 2])]


@pytest.mark.parametrize("members,js", LISTS, ids=["".join(map(str, m)) + "@" + "".join(map(str, j)) for m, j in LISTS])
def test_list_equals_single_member_reads_2_14(w14, ref14, members, js):
    w = w14
    bank = w.new_bank(3)
    got = run_list(w, bank, members, js)
    check_list(w, ref14, bank, members, js, got)
    assert np.array_equal(bank.list_result(0, len(members)), got)


def test_vm_step_equals_the_oracle_2_14(w14, ref14):
    w = w14
    members, js = [0, 0, 1, 2], [0, 1, 2, 3]
    bank = w.new_bank(3)
    got = run_list(w, bank, members, js)
    for k, (m, j) in enumerate(zip(members, js)):
        want = w.new_oram(m).read(w.o.address_new(w.addr_g[j]), w.okeys)
        assert np.array_equal(got[k], want), (k, m, j)
        w.check_word(got[k], w.data[m], j)
    check_list(w, ref14, bank, members, js, got)


# ---- 2. more entries than members: the list's digit table is its own ---------------------------------------------------------------------
def test_more_entries_than_members_2_14(w14, ref14):
    w = w14
    bank = w.new_bank(2)
    members, js = [0, 1, 0, 1, 1], [0, 1, 2, 3, 0]
    got = run_list(w, bank, members, js)
    for k, (m, j) in enumerate(zip(members, js)):
        assert np.array_equal(got[k], ref14.read(m, j)), k
    for m in range(2):
        assert_member_is(bank, m, member_snapshot(ref14.bank, m), "after the list")
    assert np.array_equal(bank.result(0, 2), got[[2, 4]])


# ---- 3. members that are not named are untouched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memo", [1, 0])
def test_a_pending_write_survives_a_list_2_14(w14, ref14, memo):
    """member 1 sits between read_prepare_write and write while a list reads members 0 and 2: its write resumes from what its
    read_prepare_write kept (trace(tree top), the rows after their alone levels in arena A, tree level 0), none of which the list touches"""
    w = w14
    config = {"memo": memo}
    bank = w.new_bank(3, config=config)
    ram = w.new_ram(1, config=config)
    a = w.addrs[1]
    vals, wct = w.words(1, seed=7)
    got = bank.read_prepare_write([a], w.keys, first=1)
    assert np.array_equal(got[0], ram.read_prepare_write(a, w.keys))
    snap = member_snapshot(bank, 1)
    members, js = [0, 2, 0], [2, 1, 3]
    got = run_list(w, bank, members, js)
    for k, (m, j) in enumerate(zip(members, js)):
        assert np.array_equal(got[k], ref14.read(m, j)), k
    assert_member_is(bank, 1, snap, "member 1 across the list")
    assert [bank.state(m) for m in range(3)] == [False, True, False]
    assert np.array_equal(bank.result(1, 1)[0], ram.result())
    bank.write(wct, [a], w.keys, first=1)
    ram.write(wct[0], a, w.keys)
    assert_member_equals_ram(bank, 1, ram, "write behind a list")
    assert np.array_equal(bank.read([a], w.keys, first=1)[0], ram.read(a, w.keys))
    for m in (0, 2):
        assert_member_is(bank, m, member_snapshot(ref14.bank, m), "named members")


# ---- 4. forced forms ---------------------------------------------------------------------------------------------------------------------
FORMS = [{"tail": 0}, {"tail_ep": 0}, {"mid": 0}, {"fuse": 0}, {"chain": 0}, {"safe": 1}, {"graph": 1}, {"tail_test": 1}, {"mid_test": 1}]
_DEFAULT_FORM = {}


def default_form(w, M, members, js):
    key = (w.max_addr, M, tuple(members), tuple(js))
    if key not in _DEFAULT_FORM:
        _DEFAULT_FORM[key] = run_list(w, w.new_bank(M), members, js).copy()
    return _DEFAULT_FORM[key]


@pytest.mark.parametrize("config", FORMS, ids=["-".join(f"{k}{v}" for k, v in c.items()) for c in FORMS])
@pytest.mark.parametrize("size", [14, 16])
def test_forced_forms_equal_the_default_form(w14, w16, size, config):
    w, M = (w14, 3) if size == 14 else (w16, 2)
    members, js = [1, 0, 1], [0, 1, 2]
    want = default_form(w, M, members, js)
    bank = w.new_bank(M, config=config)
    got = run_list(w, bank, members, js)
    assert np.array_equal(got, want), (size, config, np.count_nonzero(got != want))
    assert np.array_equal(bank.result(0, 2), got[[1, 2]])


# ---- 5. the kernels that should run, do; 10. round-off --------------------------------------------------------------------------------------
def test_list_kernels_run_2_16(w16, ref16):
    """[1, 0] at ws = 4 is 8 ciphertexts: the rows' chains of both entries are ONE k_read_chain_t launch — a permutation: the
    source map neither a batch's (all 0) nor a range's (the identity) — and the end of the read ONE k_trace_tail_t.  Four entries end in the mid chain."""
    w = w16
    rows = w.params.rows()
    bank = w.new_bank(2)
    t0 = bank.tail_stats()
    got, prof = profiled(bank, lambda: run_list(w, bank, [1, 0], [0, 1]), CLASSES)
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * 2 * w.ws, prof
    assert prof["keyswitch_tail_launch"]["launches"] == 1 and prof["keyswitch_mid_launch"]["launches"] == 0, prof
    t1 = bank.tail_stats()
    assert t1["launches"] == t0["launches"] + 1 and t1["fallbacks"] == t0["fallbacks"], (t0, t1)
    check_list(w, ref16, bank, [1, 0], [0, 1], got)
    w.check_word(got[0], w.data[1], 0)
    members, js = [1, 0, 1, 0], [0, 1, 2, 2]
    got, prof = profiled(bank, lambda: run_list(w, bank, members, js), CLASSES)
    assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * 4 * w.ws, prof
    assert prof["keyswitch_mid_launch"]["launches"] >= 1 and prof["keyswitch_tail_launch"]["launches"] == 0, prof
    ms = bank.mid_stats()
    assert ms["launches"] > 0 and ms["fallbacks"] == 0, ms
    assert bank.tail_stats() == t1
    check_list(w, ref16, bank, members, js, got)
    ro = bank.roundoff_max()   # (raises above 3/8: the call returns OK)
    print(f"roundoff_max after the 2^16 lists: {ro:.6f}")
    assert ro < 3 / 8


def test_list_tail_fallback_2_16(w16, ref16):
    """tail_test: the list's k_trace_tail_t gives up late, once, and the predicated k_read_chain_t behind it redoes coordinate 1's
    products (digits of entry y / ws) and the trace from the packed rows in the list's own arenas"""
    w = w16
    bank = w.new_bank(2, config={"tail_test": 1})
    t0 = bank.tail_stats()
    got = run_list(w, bank, [1, 0], [0, 1])
    t1 = bank.tail_stats()
    assert t1["launches"] == t0["launches"] + 1 and t1["fallbacks"] == t0["fallbacks"] + 1, (t0, t1)
    for k, (m, j) in enumerate(((1, 0), (0, 1))):
        assert np.array_equal(got[k], ref16.read(m, j)), k


# ---- 6. one row, two rows, 5-limb trace keys ---------------------------------------------------------------------------------------------------
SMALL = [(12, 4, {}, [1, 0, 0]), (13, 4, {}, [1, 0]), (13, 4, {}, [0]), (13, 2, {}, [1, 0]), (14, 4, {"k_glwe_pt": 9, "k_evk_trace": 85}, [1, 0])]
_SMALL_WORLDS = {}


def small_world(po, size, ws, crypto):
    key = (size, ws, tuple(crypto))
    if key not in _SMALL_WORLDS:
        w = World(po, 1 << size, 2, word_size=ws, seed=200 + size + ws, n_addr=3, **crypto)
        _SMALL_WORLDS[key] = (w, Ref(w, 2))
    return _SMALL_WORLDS[key]


@pytest.mark.parametrize("size,ws,crypto,members", SMALL, ids=["2p12-100", "2p13-10", "2p13-0", "2p13-ws2-10", "2p14-readme-10"])
def test_one_row_two_rows_and_readme_keys(po, size, ws, crypto, members):
    """2^12: one row, one coordinate (n2 == 1, per-entry products on the mapped rows); 2^13: two rows, and at word size 2 the list [1, 0] is
    rows * n * ws = 8 ciphertext rows, so its alone levels run as the tail chain, whose source must survive: the list's third arena (at
    word size 4 they are 16 and run as the mid chain, on two arenas); the README block: the <5, 4> instantiation of the list kernel"""
    w, ref = small_world(po, size, ws, crypto)
    bank = w.new_bank(2)
    js = list(range(len(members)))
    t0 = bank.tail_stats()
    got = run_list(w, bank, members, js)
    if (size, ws) == (13, 2):   # two tail launches: the alone levels of the rows (the third arena) and the final trace; none gave up
        t1 = bank.tail_stats()
        assert t1["launches"] == t0["launches"] + 2 and t1["fallbacks"] == t0["fallbacks"], (t0, t1)
    for k, (m, j) in enumerate(zip(members, js)):
        assert np.array_equal(got[k], ref.read(m, j)), (size, k)
        w.check_word(got[k], w.data[m], j)
    for m in range(2):
        assert bank.state(m) is False
        assert np.array_equal(bank.store_encrypted(m), ref.bank.store_encrypted(m)), m
    for m in set(members):
        last = max(k for k, mk in enumerate(members) if mk == m)
        assert np.array_equal(bank.result(m, 1)[0], got[last]), m


def test_buffer_set_walk_2_13(po):
    """The three branches of the buffer set's reserve, at the smallest shape that has them (2^13, word size 2: two rows).  One entry needs
    the result buffers only; [1, 0, 0] brings the working buffers (12 ciphertext rows: the mid chain, two arenas); [1, 0] fits the capacity
    but its 8 ciphertext rows take the tail chain, so the third arena is added and the capacity kept; [1, 0, 0] again runs on the regrown
    set.  Then the same walk through read_batch on a plain Ram: K = 1, 6, 2, 6 (K = 2 is the 8-row case: rows * K * ws = 8)."""
    w, ref = small_world(po, 13, 2, {})
    bank = w.new_bank(2)
    got = None
    for members in ([0], [1, 0, 0], [1, 0], [1, 0, 0]):
        js = list(range(len(members)))
        t0 = bank.tail_stats()
        got = run_list(w, bank, members, js)
        t1 = bank.tail_stats()
        if members == [1, 0]:   # the alone levels of the rows (on the third arena) and the final trace; none gave up
            assert t1["launches"] == t0["launches"] + 2, (t0, t1)
        assert t1["fallbacks"] == t0["fallbacks"], (members, t0, t1)
        for k, (m, j) in enumerate(zip(members, js)):
            assert np.array_equal(got[k], ref.read(m, j)), (members, k)
        got = got.copy()
    assert np.array_equal(bank.list_result(0, 3), got)
    assert np.array_equal(bank.list_result(1, 2), got[1:])
    for m in range(2):
        assert bank.state(m) is False
        assert np.array_equal(bank.store_encrypted(m), ref.bank.store_encrypted(m)), m
    ram = w.new_ram(0)
    single = [ram.read(a, w.keys).copy() for a in w.addrs]
    for m, j in ((0, 0), (0, 1), (0, 2)):   # (a bank's member is a Ram: the list's reference and the batch's agree)
        assert np.array_equal(single[j], ref.read(m, j)), j
    for sel in ([0], [0, 1, 2, 2, 1, 0], [1, 0], [0, 1, 2, 2, 1, 0]):
        t0 = ram.tail_stats()
        got = ram.read_batch([w.addrs[j] for j in sel], w.keys)
        t1 = ram.tail_stats()
        if len(sel) == 2:
            assert t1["launches"] == t0["launches"] + 2, (t0, t1)
        assert t1["fallbacks"] == t0["fallbacks"], (sel, t0, t1)
        assert got.shape[0] == len(sel)
        for k, j in enumerate(sel):
            assert np.array_equal(got[k], single[j]), (sel, k)
        assert np.array_equal(ram.result(), single[sel[-1]]), sel
    assert np.array_equal(ram.store_encrypted(), ref.bank.store_encrypted(0))


# ---- 7. derived addresses: ordered by the stream ------------------------------------------------------------------------------------------------
def test_list_behind_derive_without_a_sync_2_14(w14):
    w = w14
    pkg = w.pkg
    bank = w.new_bank(2)
    bank.read([w.addrs[0]], w.keys)   # (loads the keys)
    ks = [w.idx[0], w.idx[1]]
    fus = [pkg.FheUintPrepared.from_host(bank, w.o.fheuint_encrypt(k, 14, w.sk, 6200 + 2 * i, 6201 + 2 * i)) for i, k in enumerate(ks)]
    addrs = bank.derive_addresses(fus)
    got = bank.read_list([1, 0], addrs, w.keys).copy()           # no sync between the derive launch and the list
    bank.sync()
    again = bank.read_list([1, 0], addrs, w.keys)
    assert np.array_equal(got, again)
    for k, m in enumerate((1, 0)):
        assert np.array_equal(got[k], bank.read([addrs[k]], w.keys, first=m)[0]), k
        w.check_word(got[k], w.data[m], k)


# ---- 8. out == NULL, list_result, buffer growth and reuse ----------------------------------------------------------------------------------------
def test_enqueue_only_and_list_result_2_14(w14, ref14):
    w = w14
    bank = w.new_bank(3)
    members, js = [0, 2, 0], [0, 1, 2]
    assert run_list(w, bank, members, js, download=False) is None
    got1 = bank.read([w.addrs[3]], w.keys, first=1)[0]            # a non-list operation on another member
    assert np.array_equal(got1, ref14.read(1, 3))
    part = bank.list_result(1, 2)
    assert np.array_equal(part[0], ref14.read(2, 1)) and np.array_equal(part[1], ref14.read(0, 2))
    whole = bank.list_result(0, 3)
    check_list(w, ref14, bank, members, js, whole)
    assert np.array_equal(bank.result(1, 1)[0], got1)
    # a longer list grows the buffers, a shorter one reuses them
    members, js = [2, 1, 0, 1, 2], [3, 2, 1, 0, 0]
    check_list(w, ref14, bank, members, js, run_list(w, bank, members, js))
    members, js = [1, 2], [1, 3]
    assert run_list(w, bank, members, js, download=False) is None
    check_list(w, ref14, bank, members, js, bank.list_result(0, 2))
    with pytest.raises(w.pkg.FheRamError) as e:                  # the last list has two entries now
        bank.list_result(0, 3)
    assert e.value.code == ST_INVALID_ARG


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_lists_change_nothing_2_14(w14, ref14):
    w = w14
    pkg = w.pkg
    L = lib()
    M = 3
    bank = w.new_bank(M)
    last = run_list(w, bank, [0, 1], [0, 1]).copy()
    h = [w.addrs[j]._bank(bank) for j in range(4)]
    out = np.zeros((8, w.ws, w.params.glwe_len()), dtype=np.int64)
    snaps = [member_snapshot(bank, m) for m in range(M)]

    def c_list(members, handles, n=None, on=None, buf=out):
        n = len(members) if n is None else n
        ms = (C.c_int * max(1, len(members)))(*members)
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        return L.fheram_bank_read_list((on or bank)._h, ms, arr, n, buf.ctypes.data_as(I64P) if buf is not None else None)

    def unchanged(what):
        assert L.fheram_bank_last_error(bank._h), what
        for m in range(M):
            assert_member_is(bank, m, snaps[m], what)
        assert np.array_equal(bank.list_result(0, 2), last), what

    assert c_list([0, 1], h[:2], n=0) == ST_INVALID_ARG
    assert b"FHERAM_READ_LIST_MAX" in L.fheram_bank_last_error(bank._h)
    assert c_list([0, 1, 2] * 3, (h * 3)[:9]) == ST_INVALID_ARG
    assert b"FHERAM_READ_LIST_MAX" in L.fheram_bank_last_error(bank._h)
    unchanged("n out of range")
    assert c_list([0, -1], h[:2]) == ST_INVALID_ARG
    assert b"member -1" in L.fheram_bank_last_error(bank._h)
    assert c_list([M, 0], h[:2]) == ST_INVALID_ARG
    assert L.fheram_bank_read_list(bank._h, None, (C.c_void_p * 2)(*h[:2]), 2, None) == ST_INVALID_ARG
    assert L.fheram_bank_read_list(bank._h, (C.c_int * 2)(0, 1), None, 2, None) == ST_INVALID_ARG
    assert c_list([0, 1], [h[0], None]) == ST_INVALID_ARG
    unchanged("members / null")
    other = w.new_bank(2)
    assert c_list([0, 1], [h[0], w.addrs[0]._bank(other)]) == ST_INVALID_ARG
    assert b"does not belong" in L.fheram_bank_last_error(bank._h)
    empty = pkg.Address.alloc(bank)
    assert c_list([0, 1], [h[0], empty._bank(bank)]) == ST_INVALID_ARG
    assert b"empty address" in L.fheram_bank_last_error(bank._h)
    unchanged("foreign / empty address")
    # list_result: past the end of the last list; before any list
    assert L.fheram_bank_read_list_result(bank._h, 1, 2, out.ctypes.data_as(I64P)) == ST_INVALID_ARG
    assert L.fheram_bank_read_list_result(bank._h, 2, 1, out.ctypes.data_as(I64P)) == ST_INVALID_ARG
    assert L.fheram_bank_read_list_result(bank._h, 0, 1, None) == ST_INVALID_ARG
    assert L.fheram_bank_read_list_result(other._h, 0, 1, out.ctypes.data_as(I64P)) == ST_STATE
    unchanged("list_result")
    def no_list_yet(b):
        return L.fheram_bank_read_list_result(b._h, 0, 1, out.ctypes.data_as(I64P)) == ST_STATE

    # keys not loaded (`other` has never used any)
    other_snaps = [member_snapshot(other, m) for m in range(2)]
    assert c_list([1, 0], [w.addrs[0]._bank(other), w.addrs[1]._bank(other)], on=other) == ST_KEYS
    assert b"keys" in L.fheram_bank_last_error(other._h)
    for m in range(2):
        assert_member_is(other, m, other_snaps[m], "keys not loaded")
    assert no_list_yet(other)
    # a named member never uploaded
    partial = w.new_bank(3, load=False)
    partial.load_encrypted(0, w.rows[0])
    partial.load_encrypted(2, w.rows[2])
    last_p = run_list(w, partial, [2, 0, 2], [0, 1, 2]).copy()   # its loaded members work
    assert np.array_equal(last_p[0], ref14.read(2, 0)) and np.array_equal(last_p[2], ref14.read(2, 2))
    partial_snaps = {m: member_snapshot(partial, m) for m in (0, 2)}
    with pytest.raises(pkg.FheRamError) as e:
        run_list(w, partial, [2, 1, 0], [0, 1, 2])
    assert e.value.code == ST_UNINITIALIZED and "member 1" in e.value.msg
    for m in (0, 2):
        assert_member_is(partial, m, partial_snaps[m], "a member never uploaded")
    assert partial.state(1) is False
    with pytest.raises(pkg.FheRamError) as e:
        partial.store_encrypted(1)
    assert e.value.code == ST_UNINITIALIZED
    assert np.array_equal(partial.list_result(0, 3), last_p)
    # more than 64 ciphertexts: word size 16, five entries, on a bank that is loaded, has its keys and is given its own addresses
    p16 = pkg.Parameters(max_addr=1 << 14, word_size=16)
    wide = pkg.RamBank(p16, 2, 0)
    for m in range(2):
        wide.load_encrypted(m, np.concatenate([w.rows[m]] * 4))
    a16 = [pkg.Address(p16, list(w.addr_g[j])) for j in range(2)]
    got16 = wide.read([a16[0]], w.keys, first=1)                 # (loads the keys; four copies of member 1's words)
    assert np.array_equal(got16[0][:w.ws], ref14.read(1, 0))
    wide_snaps = [member_snapshot(wide, m) for m in range(2)]
    h16 = [a._bank(wide) for a in a16]
    assert c_list([0, 1, 0, 1, 0], [h16[0], h16[1]] * 2 + [h16[0]], on=wide) == ST_INVALID_ARG
    assert b"64" in L.fheram_bank_last_error(wide._h)
    for m in range(2):
        assert_member_is(wide, m, wide_snaps[m], "more than 64 ciphertexts")
    assert np.array_equal(wide.result(1, 1), got16) and no_list_yet(wide)
    # the Python layer refuses the same calls
    for bad in (lambda: bank.read_list([], [], w.keys), lambda: bank.read_list([0] * 9, [w.addrs[0]] * 9, w.keys),
                lambda: bank.read_list([0, 1], [w.addrs[0]], w.keys), lambda: bank.read_list([0, M], [w.addrs[0]] * 2, w.keys),
                lambda: bank.read_list([0, 1], [w.addrs[0], None], w.keys), lambda: bank.list_result(0, 0)):
        with pytest.raises(pkg.FheRamError) as e:
            bad()
        assert e.value.code == ST_INVALID_ARG
    unchanged("python layer")
    # a named member between read_prepare_write and write
    bank.read_prepare_write([w.addrs[2]], w.keys, first=1)
    snaps = [member_snapshot(bank, m) for m in range(M)]
    assert c_list([0, 1, 0], h[:3]) == ST_STATE
    assert b"member 1" in L.fheram_bank_last_error(bank._h)
    unchanged("a named member in state 1")
    # the bank that refused all of these still works
    got = run_list(w, bank, [2, 0], [1, 0])
    assert np.array_equal(got[0], ref14.read(2, 1)) and np.array_equal(got[1], ref14.read(0, 0))
    assert bank.state(1) is True
