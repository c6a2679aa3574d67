"""fheram_bank_derive_list (RamBank.derive_list, Derive) and fheram_bank_address_download (RamBank.address_digits): any mix of addresses,
selectors and selector fields from encrypted integers as ONE launch of k_cmux_jobs (include/fheram.h).

The contract, in the entry points the parent already has and in the oracle's own:
  every digit equals what fheram_bank_address_derive_at / fheram_bank_selector_derive / fheram_bank_selector_derive_fields write for the same
  integer, first bit, width and sign, and the oracle's address_from_fheuint on the integer's bits from first_bit on;
  one launch of 6 * digits workgroups, in place, ordered like the three calls; a refused call changes no target.
Every comparison is np.array_equal on int64.  Banks are at max_addr = 2^12 (four digits of three bits, one coordinate) unless a test says
otherwise: 2^13 adds a one-bit digit in a second coordinate, 2^16 a second coordinate [3, 1] whose lsh restarts."""
import ctypes as C

import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import lib, sha
from test_gpu_lanes import DATA, REGS, VALUE_B, WORD, LaneWorld, e2e_offset, e2e_setup, word_of
from test_gpu_select import ST_INVALID_ARG, VALUE, host_srcs
from test_lanes_abi import c_want

pytestmark = pytest.mark.gpu

ST_UNSUPPORTED = 5
ROWS = 6   # workgroups of a digit


class DeriveWorld(LaneWorld):
    """a LaneWorld plus the oracle's addresses from a bit offset, computed once"""

    def __init__(self, po, max_addr, n_members, word_size, seed):
        super().__init__(po, max_addr, n_members, word_size, seed)
        self._at = {}

    def addr_digits(self, value, first, sign=False):
        """address_from_fheuint on bits [first, ..) of `value`: [n_digits][ggsw_len]"""
        key = (value, first, bool(sign))
        if key not in self._at:
            self._at[key] = self.o.address_from_fheuint(self.bits(value)[first:], sign=bool(sign))
        return self._at[key]

    def fu(self, bank, value):
        return self.pkg.FheUintPrepared.from_host(bank, self.bits(value))


@pytest.fixture(scope="module")
def w2(po):
    return DeriveWorld(po, 1 << 12, 3, 2, seed=500)


@pytest.fixture(scope="module")
def w13(po):
    return DeriveWorld(po, 1 << 13, 3, 4, seed=420)   # (LaneWorld's own 2^13 world: e2e_setup / e2e_offset are shared with test_gpu_lanes.py)


@pytest.fixture(scope="module")
def w16(po):
    return DeriveWorld(po, 1 << 16, 3, 2, seed=520)


def profiled(bank, call):
    """(what call() returns, the "derive" profile of its launches)"""
    bank.sync()
    bank.profile_reset()
    bank.profile_enable(True)
    out = call()
    bank.sync()
    prof = bank.profile_get("derive")
    bank.profile_enable(False)
    return out, prof


# ---- 1. digits equal the existing calls and the oracle ---------------------------------------------------------------------------------------
def mixed_call(w, config, first_b):
    """two addresses (first bits 2 / first_b of two integers, signs 0 / 1), a plain 4-bit selector at bit 7 and a [2, 2] field selector from
    (VALUE, VALUE_B) at (0, 7) in ONE call, against the three existing calls on a second bank and against the oracle"""
    pkg, D = w.pkg, w.pkg.Derive
    n_dig = w.o.n_digits
    bank, old = w.new_bank(3, config=config), w.new_bank(3, config=config)
    fa, fb = w.fu(bank, VALUE), w.fu(bank, VALUE_B)
    plain, fsel = bank.selector(4), bank.selector_fields([2, 2])
    items = [D.address(fa, first_bit=2), D.address(fb, first_bit=first_b, sign=True), D.selector(fa, plain, first_bit=7), D.fields(fsel, [fa, fb], [0, 7])]
    targets, prof = profiled(bank, lambda: bank.derive_list(items))
    a2, ab = targets[0], targets[1]
    assert targets[2] is plain and targets[3] is fsel and targets[4] is fsel and len(targets) == 5
    digits = 2 * n_dig + plain.n_digits() + 2
    assert plain.n_digits() == 2   # the plan [3, 1]
    assert prof["launches"] == 1 and prof["blocks"] == ROWS * digits, prof
    # the existing entry points, on a bank of their own
    oa, ob = w.fu(old, VALUE), w.fu(old, VALUE_B)
    o2, = old.derive_addresses([oa], first_bits=[2])
    o18, = old.derive_addresses([ob], sign=True, first_bits=[first_b])
    oplain, = old.derive_selectors([oa], [7], [old.selector(4)])
    ofsel = old.derive_selector_fields(old.selector_fields([2, 2]), [oa, ob], [0, 7])
    got = {"a2": bank.address_digits(a2), "ab": bank.address_digits(ab), "plain": plain.download(), "fields": fsel.download()}
    assert got["a2"].shape == (n_dig, w.params.ggsw_len())
    assert np.array_equal(got["a2"], old.address_digits(o2)) and np.array_equal(got["ab"], old.address_digits(o18))
    assert np.array_equal(got["plain"], oplain.download()) and np.array_equal(got["fields"], ofsel.download())
    # the oracle
    assert np.array_equal(got["a2"], w.addr_digits(VALUE, 2, False)), "address at bit 2"
    assert np.array_equal(got["ab"], w.addr_digits(VALUE_B, first_b, True)), "address with sign = 1"
    assert np.array_equal(got["plain"], w.digits(VALUE, 7, 4)), "plain selector"
    assert np.array_equal(got["fields"], w.field_digits([2, 2], (VALUE, VALUE_B), (0, 7))), "field selector"
    # a read list and a select through the targets
    lst = bank.read_list([1, 2], [a2, ab], w.keys)
    assert np.array_equal(lst[0], w.new_oram(1).read(w.o.address_new(got["a2"]), w.okeys))
    assert np.array_equal(lst[1], w.new_oram(2).read(w.o.address_new(got["ab"]), w.okeys))
    vals, cts = w.candidates(16, seed=60)
    out = bank.select([plain, fsel], [host_srcs(pkg, 16)] * 2, host_words=cts)
    assert np.array_equal(out[0], w.oselect(4, cts, got["plain"]))
    assert np.array_equal(out[1], w.oselect_fields([2, 2], cts, got["fields"]))
    w.check_value(out[0], vals[(VALUE >> 7) & 15], "plain selector")
    w.check_value(out[1], vals[(VALUE & 3) | (((VALUE_B >> 7) & 3) << 2)], "field selector")
    return bank


def test_digits_equal_the_existing_calls_and_the_oracle(w2):
    mixed_call(w2, None, 18)


def test_digits_at_2p16_where_lsh_restarts(w16):
    """the plan [[3, 3, 3, 3], [3, 1]]: coordinate 1 restarts lsh, and chains of 3, 2, 1 bits sit side by side.  (16 address bits: the second
    address starts at bit 16 of its 32-bit integer, not at 18)"""
    assert w16.o.n_digits == 6
    mixed_call(w16, None, 16)


# ---- 7. forced forms ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [{"safe": 1}, {"monitor": 2}], ids=["safe", "monitor2"])
def test_forced_forms_give_the_same_integers(w2, config):
    bank = mixed_call(w2, config, 18)
    ro = bank.roundoff_max()
    print(f"derive list under {config}: round-off maximum {ro:.4f}")
    assert ro < 0.375


# ---- 2. in place --------------------------------------------------------------------------------------------------------------------------------
def test_in_place_over_every_kind_of_target(w2):
    """targets from Address.alloc, host digits, _create_fields, earlier derivations by the old calls and by a derive list; a second derive list
    then changes only some of them"""
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    bank = w.new_bank(1)
    fa, fb = w.fu(bank, VALUE), w.fu(bank, VALUE_B)
    blank = pkg.Address.alloc(bank)
    host = pkg.Address(w.params, list(w.addr_g[0]))
    made = pkg.Selector.from_digits_fields(bank, [2, 2], list(w.field_digits([2, 2], (VALUE_B, VALUE), (3, 11))))
    by_old, = bank.derive_addresses([fb], first_bits=[9])
    sel_old, = bank.derive_selectors([fb], [3], [bank.selector(3)])
    by_list, sel_list = bank.derive_list([D.address(fa, first_bit=20), D.selector(fb, bank.selector(5), first_bit=1)])
    assert np.array_equal(bank.address_digits(by_list), w.addr_digits(VALUE, 20)) and np.array_equal(sel_list.download(), w.digits(VALUE_B, 1, 5))
    got = bank.derive_list([D.address(fa, blank, 0), D.address(fb, host, 4, sign=True), D.fields(made, [fa, fb], [0, 7]), D.address(fa, by_old, 11),
                            D.selector(fa, sel_old, 29), D.address(fb, by_list, 2), D.selector(fa, sel_list, 7)])
    assert got[0] is blank and got[1] is host and got[2] is made and got[3] is made and got[4] is by_old and got[7] is sel_list
    want = {"blank": w.addr_digits(VALUE, 0), "host": w.addr_digits(VALUE_B, 4, True), "made": w.field_digits([2, 2], (VALUE, VALUE_B), (0, 7)),
            "by_old": w.addr_digits(VALUE, 11), "sel_old": w.digits(VALUE, 29, 3), "by_list": w.addr_digits(VALUE_B, 2), "sel_list": w.digits(VALUE, 7, 5)}

    def state():
        return {"blank": bank.address_digits(blank), "host": bank.address_digits(host), "made": made.download(), "by_old": bank.address_digits(by_old),
                "sel_old": sel_old.download(), "by_list": bank.address_digits(by_list), "sel_list": sel_list.download()}

    have = state()
    for k in want:
        assert np.array_equal(have[k], want[k]), k
    before = {k: sha(v) for k, v in have.items()}
    bank.derive_list([D.address(fb, host, 20), D.selector(fb, sel_old, 0), D.fields(made, [fb, fb], [1, 30])])
    have = state()
    assert np.array_equal(have["host"], w.addr_digits(VALUE_B, 20)) and np.array_equal(have["sel_old"], w.digits(VALUE_B, 0, 3))
    assert np.array_equal(have["made"], w.field_digits([2, 2], (VALUE_B, VALUE_B), (1, 30)))
    for k in ("blank", "by_old", "by_list", "sel_list"):
        assert sha(have[k]) == before[k], (k, "a target the second list did not name changed")
    assert np.array_equal(bank.read([blank], w.keys)[0], w.new_oram(0).read(w.o.address_new(want["blank"]), w.okeys))


# ---- 3. one integer feeding every item ---------------------------------------------------------------------------------------------------------
def test_one_integer_feeds_five_fields_and_a_plain_selector(w2):
    """five one-bit fields from bits 0..4 of one integer are the plain 5-bit selector's index: a select over 32 host candidates picks the same word"""
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    bank = w.new_bank(1)
    bank._use_keys(w.keys)
    fa = w.fu(bank, VALUE)
    ones, plain = bank.selector_fields([1] * 5), bank.selector(5)
    (_, prof) = profiled(bank, lambda: bank.derive_list([D.fields(ones, [fa] * 5, [0, 1, 2, 3, 4]), D.selector(fa, plain)]))
    assert prof["launches"] == 1 and prof["blocks"] == ROWS * (5 + 2), prof
    padded = [1, 1, 1, 1, 1, 1, 3, 3]   # a DECOMP_N that starts with the five widths (as LaneWorld.field_oracle pads them)
    assert w.po.get_base_2d(32, padded) == [[1] * 5]
    ob = w.po.Oracle(w.po.OParams(max_addr=32, word_size=w.ws, decomp_n=padded))
    assert np.array_equal(ones.download(), ob.address_from_fheuint(w.bits(VALUE)[:5], sign=False))
    assert np.array_equal(plain.download(), w.digits(VALUE, 0, 5))
    by_old = bank.derive_selector_fields(bank.selector_fields([1] * 5), [fa] * 5, [0, 1, 2, 3, 4])
    assert np.array_equal(ones.download(), by_old.download())
    vals, cts = w.candidates(32, seed=50)
    got_fields = bank.select([ones], [host_srcs(pkg, 32)], host_words=cts)[0]
    got_plain = bank.select([plain], [host_srcs(pkg, 32)], host_words=cts)[0]
    assert np.array_equal(got_plain, w.oselect(5, cts, w.digits(VALUE, 0, 5)))
    for got in (got_fields, got_plain):
        w.check_value(got, vals[VALUE & 31], "index = bits [0, 5)")


# ---- 4. more workgroups than CUs, and the limit ---------------------------------------------------------------------------------------------
COMBOS = [(VALUE, 2, False), (VALUE_B, 0, True), (VALUE, 18, True), (VALUE_B, 11, False)]   # (integer, first bit, sign)


def test_more_workgroups_than_compute_units(w13):
    """2^13: five digits ([3, 3, 3, 3] and [1]).  Eight addresses and a five-field selector are 45 jobs, 270 workgroups: a second round, which the
    one-bit chains fill (the host orders the jobs by descending width)"""
    w, pkg, D = w13, w13.pkg, w13.pkg.Derive
    assert w.o.n_digits == 5
    bank, old = w.new_bank(1), w.new_bank(1)
    f = {VALUE: w.fu(bank, VALUE), VALUE_B: w.fu(bank, VALUE_B)}
    g = {VALUE: w.fu(old, VALUE), VALUE_B: w.fu(old, VALUE_B)}
    specs = [COMBOS[i % 4] if i < 4 else (COMBOS[i % 4][0], COMBOS[i % 4][1] + 1, COMBOS[i % 4][2]) for i in range(8)]
    ones = bank.selector_fields([1] * 5)
    firsts = [31, 0, 17, 4, 9]
    fus = [VALUE, VALUE_B, VALUE, VALUE, VALUE_B]
    items = [D.address(f[v], first_bit=fb, sign=s) for v, fb, s in specs[:5]] + [D.fields(ones, [f[v] for v in fus], firsts)] + \
            [D.address(f[v], first_bit=fb, sign=s) for v, fb, s in specs[5:]]   # (the fields in the middle of the list)
    targets, prof = profiled(bank, lambda: bank.derive_list(items))
    assert prof["launches"] == 1 and prof["blocks"] == ROWS * 45 == 270, prof
    addrs = targets[:5] + targets[10:]
    for sign in (False, True):   # the single derivations: the old call takes one sign per call
        idx = [i for i in range(8) if specs[i][2] == sign]
        olds = old.derive_addresses([g[specs[i][0]] for i in idx], sign=sign, first_bits=[specs[i][1] for i in idx])
        for i, o in zip(idx, olds):
            d = bank.address_digits(addrs[i])
            assert np.array_equal(d, old.address_digits(o)), (i, specs[i])
            assert np.array_equal(d, w.addr_digits(*specs[i])), (i, specs[i])
    oones = old.derive_selector_fields(old.selector_fields([1] * 5), [g[v] for v in fus], firsts)
    assert np.array_equal(ones.download(), oones.download())


def test_sixty_four_digits_work_and_sixty_five_are_refused(w13):
    w, pkg, D = w13, w13.pkg, w13.pkg.Derive
    bank = w.new_bank(1)
    f = {VALUE: w.fu(bank, VALUE), VALUE_B: w.fu(bank, VALUE_B)}
    addrs = [pkg.Address.alloc(bank) for _ in range(12)]
    pairs = [bank.selector_fields([1, 1]) for _ in range(2)]
    one = bank.selector(1)
    bank.derive_list([D.selector(f[VALUE], one, 13)])
    full = [D.address(f[COMBOS[i % 4][0]], addrs[i], COMBOS[i % 4][1], COMBOS[i % 4][2]) for i in range(12)] + \
           [D.fields(pairs[0], [f[VALUE], f[VALUE_B]], [0, 7]), D.fields(pairs[1], [f[VALUE_B], f[VALUE]], [30, 31])]
    (_, prof) = profiled(bank, lambda: bank.derive_list(full))
    assert prof["launches"] == 1 and prof["blocks"] == ROWS * 64, prof   # 12 * 5 + 2 * 2
    for i in range(12):
        assert np.array_equal(bank.address_digits(addrs[i]), w.addr_digits(*COMBOS[i % 4])), i
    padded = [1, 1, 2, 2, 3, 3]
    assert w.po.get_base_2d(4, padded) == [[1, 1]]
    ob = w.po.Oracle(w.po.OParams(max_addr=4, word_size=w.ws, decomp_n=padded))
    two = lambda va, fa, vb, fb: ob.address_from_fheuint(np.concatenate([w.bits(va)[fa:fa + 1], w.bits(vb)[fb:fb + 1]]), sign=False)   # noqa: E731
    assert np.array_equal(pairs[0].download(), two(VALUE, 0, VALUE_B, 7)) and np.array_equal(pairs[1].download(), two(VALUE_B, 30, VALUE, 31))

    def digest():
        return [sha(bank.address_digits(a)) for a in addrs] + [sha(p.download()) for p in pairs] + [sha(one.download())]

    before = digest()
    moved = [D.address(f[COMBOS[(i + 1) % 4][0]], addrs[i], COMBOS[(i + 1) % 4][1], COMBOS[(i + 1) % 4][2]) for i in range(12)] + \
            [D.fields(pairs[0], [f[VALUE_B], f[VALUE]], [3, 4]), D.fields(pairs[1], [f[VALUE], f[VALUE]], [5, 6]), D.selector(f[VALUE_B], one, 2)]
    with pytest.raises(pkg.FheRamError) as e:
        bank.derive_list(moved)
    assert e.value.code == ST_INVALID_ARG and "65" in e.value.msg and "FHERAM_DERIVE_LIST_DIGITS_MAX" in e.value.msg, e.value
    assert digest() == before, "a refused call changed a target"
    bank.derive_list(moved[:-1])   # the same without the 65th digit
    assert np.array_equal(bank.address_digits(addrs[11]), w.addr_digits(*COMBOS[0]))


# ---- 5. ordering, on a bank of one member (a plain context: pre_inv is live) -----------------------------------------------------------------
@pytest.mark.parametrize("config", [None, {"memo": 0}], ids=["default", "memo0"])
def test_derive_list_between_read_prepare_write_and_write(w2, config):
    """stale memo / pre_inv state: the write must not resume from the inverse digits started early for the OLD digits of the handle"""
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    vals, cts = w.candidates(3)
    bank = w.new_bank(1, config=config)
    fa, fb = w.fu(bank, VALUE), w.fu(bank, VALUE_B)
    a, = bank.derive_list([D.address(fa, first_bit=2)])
    got_rpw = bank.read_prepare_write([a], w.keys).copy()
    bank.derive_list([D.address(fb, a, first_bit=5)])
    bank.write(cts[0:1], [a], w.keys)
    ref = w.new_bank(1, config=config)
    a1, a2 = pkg.Address(w.params, list(w.addr_digits(VALUE, 2))), pkg.Address(w.params, list(w.addr_digits(VALUE_B, 5)))
    want_rpw = ref.read_prepare_write([a1], w.keys).copy()
    ref.write(cts[0:1], [a2], w.keys)
    assert np.array_equal(got_rpw, want_rpw)
    assert bank.state(0) == ref.state(0) and not bank.state(0)
    assert np.array_equal(bank.store_encrypted(0), ref.store_encrypted(0)), "rows after the write"
    assert np.array_equal(bank.read([a], w.keys), ref.read([a2], w.keys))


def test_derive_list_read_prepare_write_select_write_without_a_sync(w2):
    """derive list, read_prepare_write, select and write_list_selected back to back, nothing downloaded in between: the side work read_prepare_write
    starts early reads the address's digits behind the derive launch"""
    w, pkg, D, S = w2, w2.pkg, w2.pkg.Derive, w2.pkg.Src
    vals, cts = w.candidates(3)
    bank = w.new_bank(1)
    bank._use_keys(w.keys)
    fa, fb = w.fu(bank, VALUE), w.fu(bank, VALUE_B)
    a, sel = pkg.Address.alloc(bank), bank.selector(1)
    bank.sync()
    bank.derive_list([D.address(fa, a, 2), D.selector(fb, sel, 9)])
    bank.read_prepare_write([a], w.keys, download=False)
    assert bank.select([sel], [[S.member(0), S.host(1)]], host_words=cts, download=False) is None
    bank.write_list_selected([0], [0], [a], w.keys)
    ref = w.new_bank(1)
    ra = pkg.Address(w.params, list(w.addr_digits(VALUE, 2)))
    old = ref.read_prepare_write([ra], w.keys).copy()
    pick = ref.select([pkg.Selector.from_digits(ref, 1, list(w.digits(VALUE_B, 9, 1)))], [[S.member(0), S.host(1)]], host_words=cts)
    ref.write(pick, [ra], w.keys)
    assert np.array_equal(bank.result(0, 1), old) and np.array_equal(bank.select_result(0, 1), pick)
    assert np.array_equal(pick[0], w.oselect(1, np.stack([old[0], cts[1]]), w.digits(VALUE_B, 9, 1)))
    assert np.array_equal(bank.store_encrypted(0), ref.store_encrypted(0)), "rows after the write"
    assert bank.state(0) is False   # (2^12: one row per sub-RAM, no tree level)
    assert bank.roundoff_max() < 0.375


def test_derive_read_derive_read_on_one_handle(w2):
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    bank = w.new_bank(1)
    fa, fb = w.fu(bank, VALUE), w.fu(bank, VALUE_B)
    a, = bank.derive_list([D.address(fa, first_bit=2)])
    r1 = bank.read([a], w.keys)[0].copy()
    bank.derive_list([D.address(fb, a, first_bit=2)])
    r2 = bank.read([a], w.keys)[0].copy()
    bank.derive_list([D.address(fa, a, first_bit=2)])
    r3 = bank.read([a], w.keys)[0].copy()
    oread = lambda v: w.new_oram(0).read(w.o.address_new(w.addr_digits(v, 2)), w.okeys)   # noqa: E731
    assert np.array_equal(r1, oread(VALUE)), "first read"
    assert np.array_equal(r2, oread(VALUE_B)), "read after the address was overwritten in place"
    assert np.array_equal(r3, r1) and not np.array_equal(r1, r2)


# ---- 6. the step end to end at 2^13 ------------------------------------------------------------------------------------------------------------
def e2e_run_list(w, cands_of, op, offset, y_from_read):
    """e2e_run of test_gpu_lanes.py with its two derivation calls replaced by ONE derive list: the address from bits [2, ..) of the byte address and
    the [2, 2] selector from `op` and the address's low bits"""
    pkg, S, D = w.pkg, w.pkg.Src, w.pkg.Derive
    byte_addr, digits, old = e2e_offset(w, offset)
    bank = w.new_bank(3)
    fu_addr = pkg.FheUintPrepared.from_host(bank, w.bits(byte_addr))
    fu_op = pkg.FheUintPrepared.from_host(bank, w.bits(op))
    sel = bank.selector_fields([2, 2])
    (targets, prof) = profiled(bank, lambda: bank.derive_list([D.address(fu_addr, first_bit=2), D.fields(sel, [fu_op, fu_addr], [0, 0])]))
    assert prof["launches"] == 1 and prof["blocks"] == ROWS * (5 + 2), prof
    addr = targets[0]
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


@pytest.mark.parametrize("offset,op", [(0, 0), (1, 1), (2, 2), (0, 3)])
def test_store_step_end_to_end(w13, offset, op):
    w, pkg = w13, w13.pkg
    s = e2e_setup(w)
    bank, addr, digits, old = e2e_run_list(w, lambda x, y: pkg.store_merge_lanes(x, y), op, offset, False)
    assert np.array_equal(bank.address_digits(addr), digits)
    cands = pkg.store_merge_lanes(pkg.Src.list(0), pkg.Src.member(DATA))
    words = w.assemble(cands, {(3, 0): s["x"], (2, DATA): old})
    pick = w.oselect_fields([2, 2], words, w.field_digits([2, 2], (op, (WORD << 2) | offset), (0, 0)))
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
    w.check_value(back, [(want >> (8 * i)) & 0xFF for i in range(4)], (offset, op))
    for m in (REGS, 1):
        assert np.array_equal(np.ravel(bank.store_encrypted(m)), np.ravel(w.rows[m])), "a member that was not written changed"


def test_load_step_end_to_end(w13):
    """LHU at offset 2: the data word's upper half, zero-extended, lands in the register file"""
    w, pkg = w13, w13.pkg
    offset, op = 2, 2
    s = e2e_setup(w)
    bank, addr, digits, _ = e2e_run_list(w, lambda y: pkg.load_extract_lanes(y), op, offset, True)
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
    w.check_value(back, [s["ybytes"][2], s["ybytes"][3], 0, 0], "LHU at offset 2")
    for m in (DATA, 1):
        assert np.array_equal(np.ravel(bank.store_encrypted(m)), np.ravel(w.rows[m])), "a member that was not written changed"


# ---- 8. refusals: every one before anything is enqueued ---------------------------------------------------------------------------------------
def test_refusals_change_no_target(w2):
    w, pkg, D = w2, w2.pkg, w2.pkg.Derive
    A = pkg.api
    lb = lib()
    bank, other = w.new_bank(1), w.new_bank(1)
    fa, fb = w.fu(bank, VALUE), w.fu(bank, VALUE_B)
    fu10 = pkg.FheUintPrepared.from_host(bank, w.bits(VALUE)[:10])
    fu_other = w.fu(other, VALUE)
    a, b = pkg.Address.alloc(bank), pkg.Address.alloc(bank)
    plain, fsel = bank.selector(4), bank.selector_fields([2, 2])
    a_other, plain_other, fsel_other = pkg.Address.alloc(other), other.selector(4), other.selector_fields([2, 2])
    valid = [D.address(fa, a, 2), D.address(fb, b, 18, sign=True), D.selector(fa, plain, 7), D.fields(fsel, [fa, fb], [0, 7])]

    def digest():
        return [sha(bank.address_digits(a)), sha(bank.address_digits(b)), sha(plain.download()), sha(fsel.download())]

    bank.derive_list(valid)
    good = digest()
    assert good[0] == sha(w.addr_digits(VALUE, 2)) and good[3] == sha(w.field_digits([2, 2], (VALUE, VALUE_B), (0, 7)))
    ha, hb = a._bank(bank), b._bank(bank)

    def item(kind, fu, target, first_bit=0, sign=0, field=0):
        return A._CDeriveItem(kind, first_bit, sign, field, fu, target)

    ADDR, SEL, FIELD = A.DERIVE_ADDRESS, A.DERIVE_SELECTOR, A.DERIVE_FIELD
    # every refused list also names targets with a derivation that WOULD change them (other first bits than `valid`)
    moved = [item(ADDR, fb._h, ha, 3), item(ADDR, fa._h, hb, 1), item(SEL, fb._h, plain._h, 11), item(FIELD, fb._h, fsel._h, 5, 0, 0), item(FIELD, fa._h, fsel._h, 9, 0, 1)]

    def refused(what, items, code=ST_INVALID_ARG, n=None, say=None, bank_h=None):
        arr = (A._CDeriveItem * max(len(items), 1))(*items)
        rc = lb.fheram_bank_derive_list(bank._h if bank_h is None else bank_h, arr if items else None, len(items) if n is None else n)
        assert rc == code, (what, rc)
        msg = lb.fheram_bank_last_error(bank._h).decode()
        assert msg, what
        if say:
            assert say in msg, (what, msg)
        assert digest() == good, (what, "a refused call changed a target")
        bank.derive_list(valid)   # ... and the bank still derives
        assert digest() == good, (what, "the call after a refusal")

    refused("null items", [], n=1)
    refused("n = 0", moved, n=0, say="FHERAM_DERIVE_LIST_MAX")
    refused("n = 33", (moved * 7)[:33], say="FHERAM_DERIVE_LIST_MAX")
    refused("n = -1", moved, n=-1)
    refused("unknown kind", moved + [item(3, fa._h, plain._h)], say="item 5")
    refused("negative kind", [item(-1, fa._h, ha)] + moved[1:], say="item 0")
    refused("null integer", moved[:2] + [item(SEL, None, plain._h, 11)], say="item 2")
    refused("integer of another bank", moved[:1] + [item(ADDR, fu_other._h, hb, 1)], say="item 1")
    refused("null target", moved[:1] + [item(ADDR, fa._h, None, 1)], say="item 1")
    refused("address of another bank", moved[:1] + [item(ADDR, fa._h, a_other._bank(other), 1)], say="item 1")
    refused("plain selector of another bank", moved[:2] + [item(SEL, fa._h, plain_other._h, 1)], say="item 2")
    refused("field selector of another bank", moved[:2] + [item(FIELD, fa._h, fsel_other._h, 1)], say="item 2")
    refused("sign on a plain selector", moved[:2] + [item(SEL, fb._h, plain._h, 11, sign=1)], say="item 2")
    refused("sign on a field", moved[:3] + [item(FIELD, fb._h, fsel._h, 5, 1, 0), moved[4]], say="item 3")
    refused("field on an address", moved[:1] + [item(ADDR, fa._h, hb, 1, 0, 1)] + moved[2:], say="item 1")
    refused("field on a plain selector", moved[:2] + [item(SEL, fb._h, plain._h, 11, 0, 1)], say="item 2")
    refused("negative first bit", moved[:1] + [item(ADDR, fa._h, hb, -1)], say="item 1")
    refused("address bits beyond the integer", moved[:1] + [item(ADDR, fa._h, hb, 21)], say="item 1")
    refused("address from a narrow integer", moved[:1] + [item(ADDR, fu10._h, hb, 0)], say="item 1")
    refused("selector bits beyond the integer", moved[:2] + [item(SEL, fb._h, plain._h, 29)], say="item 2")
    refused("field bits beyond the integer", moved[:4] + [item(FIELD, fa._h, fsel._h, 31, 0, 1)], say="item 4")
    refused("field bits beyond a narrow integer", moved[:4] + [item(FIELD, fu10._h, fsel._h, 9, 0, 1)], say="item 4")
    refused("an address twice", moved[:2] + [item(ADDR, fa._h, ha, 5)], say="item 2")
    refused("a plain selector twice", moved[:3] + [item(SEL, fa._h, plain._h, 3)], say="item 3")
    refused("SELECTOR naming a field selector", moved[:2] + [item(SEL, fb._h, fsel._h, 11)], say="item 2")
    refused("FIELD naming a plain selector", moved[:2] + [item(FIELD, fb._h, plain._h, 11)], say="item 2")
    refused("field = 2 of two", moved[:4] + [item(FIELD, fa._h, fsel._h, 9, 0, 2)], say="item 4")
    refused("field = -1", moved[:4] + [item(FIELD, fa._h, fsel._h, 9, 0, -1)], say="item 4")
    refused("a field selector in part", moved[:4], say="not all")
    refused("one field twice", moved[:4] + [item(FIELD, fa._h, fsel._h, 9, 0, 0)], say="item 4")
    refused("one field twice beside the whole", moved + [item(FIELD, fa._h, fsel._h, 1, 0, 1)], say="item 5")
    probe = np.zeros((4, w.params.ggsw_len()), dtype=np.int64)
    p = probe.ctypes.data_as(C.POINTER(C.c_int64))
    assert lb.fheram_bank_address_download(bank._h, ha, None) == ST_INVALID_ARG
    assert lb.fheram_bank_address_download(bank._h, None, p) == ST_INVALID_ARG
    assert lb.fheram_bank_address_download(bank._h, a_other._bank(other), p) == ST_INVALID_ARG
    assert lb.fheram_bank_address_download(bank._h, pkg.Address.alloc(bank)._bank(bank), p) == ST_INVALID_ARG   # an empty address
    assert not probe.any()
    with pytest.raises(pkg.FheRamError) as e:   # through the mirror, which allocates the address of an addr=None item and drops it again
        bank.derive_list([D.address(fb, a, 3), D.address(fa, first_bit=40)])
    assert e.value.code == ST_INVALID_ARG and "item 1" in e.value.msg and digest() == good
    # a refused list leaves an empty target empty
    blank, blank_sel = pkg.Address.alloc(bank), bank.selector(2)
    refused("empty targets in a refused list", [item(ADDR, fa._h, blank._bank(bank), 2), item(SEL, fa._h, blank_sel._h, 1), item(ADDR, fa._h, ha, 40)], say="item 2")
    assert lb.fheram_bank_address_download(bank._h, blank._bank(bank), p) == ST_INVALID_ARG
    with pytest.raises(pkg.FheRamError):
        blank_sel.download()
    # the whole field selector beside everything else is accepted
    assert lb.fheram_bank_derive_list(bank._h, (A._CDeriveItem * 5)(*moved), 5) == 0
    assert np.array_equal(fsel.download(), w.field_digits([2, 2], (VALUE_B, VALUE), (5, 9))) and np.array_equal(bank.address_digits(a), w.addr_digits(VALUE_B, 3))


def test_a_nine_digit_plan_is_refused(po):
    """an address plan of more than 8 digits: FHERAM_ERR_UNSUPPORTED as fheram_address_derive refuses it; selectors alone are still derived"""
    pkg = load_package()
    D = pkg.Derive
    plan, max_addr = [2, 2, 2, 1, 1, 1, 1, 1, 1], 1 << 12
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=1, decomp_n=plan))
    sk = o.secret_gen(41)
    params = pkg.Parameters(max_addr=max_addr, word_size=1, decomp_n=plan)
    assert params.base2d().as_1d().size() == 9
    bank = pkg.RamBank(params, 1, 0)
    before = o.address_encrypt(777, sk, 42, 43)
    a = pkg.Address(params, list(before))
    bits = o.fheuint_encrypt(1234, 12, sk, 44, 45)
    fu = pkg.FheUintPrepared.from_host(bank, bits)
    sel = bank.selector(2)
    with pytest.raises(pkg.FheRamError) as e:
        bank.derive_list([D.selector(fu, sel, 3), D.address(fu, a)])
    assert e.value.code == ST_UNSUPPORTED and "8 digits" in e.value.msg, (e.value.code, e.value.msg)
    assert np.array_equal(bank.address_digits(a), before)
    with pytest.raises(pkg.FheRamError):   # still empty
        sel.download()
    bank.derive_list([D.selector(fu, sel, 3)])
    small = po.Oracle(po.OParams(max_addr=4, word_size=1, decomp_n=plan))
    assert np.array_equal(sel.download(), small.address_from_fheuint(bits[3:5], sign=False))
