"""Adversarial operands THROUGH the kernels of the operations on several addresses: k_cmux_chain (fheram_address_derive) and the table forms
k_read_chain_t / k_write_chain_t / k_trace_tail_t with its k_read_chain_t fallback and the mid chain over a range (fheram_bank,
fheram_bank_read_list, fheram_read_batch).  tests/test_gpu_extremes.py feeds limbs at the ends of the normalised range — every limb -2^16,
every limb 2^16 - 1, alternating, one coefficient flipped, random signs — to the single-context chains; here the same limbs go through the
kernels that take an operand table, with a DIFFERENT kind per member, address or integer, so that a kernel that fetched member 1's operand
for member 0 cannot pass.

Nothing here is a valid ciphertext: nothing decrypts, everything compares — np.array_equal against the oracle (exact integer arithmetic),
no tolerance anywhere.  The precondition of the exactness contract (every post-inverse-transform value below 2^47: SURVEY.md A.9, DESIGN.md
11) is asserted on the oracle's side for every flow: the oracle records the largest |coefficient| behind each inverse transform, i.e. of the
whole sum of an output limb (vmp_to_big: all 8 terms of a CMux step's limb, all 6 of an external product's), which is what k_cmux_chain
inverts.  No case had to be dropped for exceeding it.  The round-off monitor runs on every coefficient (monitor = 2) and must stay inside
(0, 3/8), the library's own limit (FHERAM_ERR_PRECISION); the maxima are printed."""
import zlib

import numpy as np
import pytest

from _pkg import load_package
from test_gpu_bank import CLASSES, assert_member_is, member_snapshot, profiled
from test_gpu_extremes import N, PATTERNS, _fill, _threads

pytestmark = pytest.mark.gpu

KINDS = ["lo", "hi", "alternating", "flipped", "signs"]
assert {k for p in PATTERNS for k in p} == set(KINDS)
PRECISION = 3 / 8   # MON_LIMIT: above it the library returns FHERAM_ERR_PRECISION


def _rng(*what):
    return np.random.default_rng(zlib.crc32("/".join(str(x) for x in what).encode()))


# =====================================================================================================================================
# A. k_cmux_chain: encrypted integers of extreme limbs
# =====================================================================================================================================
# (max_addr, digit plan), all at word size 1: the default plan; one chain of 12 steps (rotations up to 2^11); two of 6; three of 4; a size
# that is no power of two, with chains of unequal length (5, 4, 3 and the 1-bit digit of coordinate 1) in one launch
DERIVE_SHAPES = [(1 << 14, (3, 3, 3, 3)), (1 << 13, (12,)), (1 << 13, (6, 6)), (1 << 14, (4, 4, 4)), (5000, (5, 4, 3))]
_DERIVE_WORLDS = {}
_DERIVE_RO = {}


def got_digits(addr):
    addr._digits = None   # (always from the device)
    return np.stack(addr.digits)


def mixed_integer(w, seed):
    """an integer whose bits are of different kinds: bit i of kind KINDS[(i + seed) % 5]"""
    return np.concatenate([_fill(KINDS[(i + seed) % len(KINDS)], (1, w.flen), _rng("mixed", seed, i)) for i in range(w.n_bits)])


class DeriveWorld:
    """One oracle context and one Ram (every coefficient monitored) of a shape; the "encrypted integers" [n_bits][fheuint_ggsw_len] of each
    kind and the digits the oracle derives from them, computed once."""

    def __init__(self, po, max_addr, plan):
        pkg = load_package()
        self.pkg, self.max_addr, self.plan = pkg, max_addr, plan
        self.o = po.Oracle(po.OParams(max_addr=max_addr, word_size=1, decomp_n=list(plan)))
        self.params = pkg.Parameters(max_addr=max_addr, word_size=1, decomp_n=list(plan))
        self.n_bits = sum(sum(b.d) for b in self.params.base2d().v)   # the bits the plan reads (conversion.rs:45-62)
        self.flen = self.o.fheuint_ggsw_len()
        self.ram = pkg.Ram(self.params, 0, config={"monitor": 2})
        self._bits, self._digits = {}, {}

    def bits(self, kind):
        if kind not in self._bits:
            if kind.startswith("mixed"):
                self._bits[kind] = mixed_integer(self, int(kind[5:]))
            elif kind.startswith("signs"):
                self._bits[kind] = _fill("signs", (self.n_bits, self.flen), _rng(kind, self.max_addr, self.plan))
            else:
                self._bits[kind] = _fill(kind, (self.n_bits, self.flen), None)
        return self._bits[kind]

    def digits(self, kind, sign):
        """Oracle.address_from_fheuint, with the precondition of the exactness contract asserted for this very derivation"""
        if (kind, sign) not in self._digits:
            self.o.reset_stats()
            self._digits[(kind, sign)] = self.o.address_from_fheuint(self.bits(kind), sign=sign)
            big = self.o.max_big()
            assert big < 1 << 47, (self.max_addr, self.plan, kind, sign, big)   # a condition of the contract, not a measurement
        return self._digits[(kind, sign)]


def derive_world(po, max_addr, plan):
    if (max_addr, plan) not in _DERIVE_WORLDS:
        _DERIVE_WORLDS.clear()   # (one shape's integers at a time: the cases of a shape run back to back)
        _DERIVE_WORLDS[(max_addr, plan)] = DeriveWorld(po, max_addr, plan)
    return _DERIVE_WORLDS[(max_addr, plan)]


def _shape_id(s):
    return f"{s[0]}-" + "_".join(map(str, s[1]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", DERIVE_SHAPES, ids=_shape_id)
def test_extreme_integers_through_the_cmux_chain(po, shape, kind):
    """Ram.derive_addresses (ONE k_cmux_chain launch: the 8 terms of an output limb summed in the transform domain, inverted once, int
    carries) against the oracle AND against the unchanged Address.set_from_fheuint (every term inverted on its own) on the same operands,
    both signs.  Cases dropped for exceeding 2^47: none."""
    w = derive_world(po, *shape)
    pkg, ram = w.pkg, w.ram
    fu = pkg.FheUintPrepared.from_host(ram, w.bits(kind))
    n_digits = w.params.base2d().as_1d().size()
    for sign in (False, True):
        want = w.digits(kind, sign)
        ram.roundoff_reset()
        ram.profile_enable(True)
        ram.profile_reset()
        addr, = ram.derive_addresses([fu], sign=sign)
        prof = ram.profile_get("derive")
        ram.profile_enable(False)
        ro = ram.roundoff_max(check=False)           # of the derive launch alone
        got = got_digits(addr)
        _DERIVE_RO[shape] = max(_DERIVE_RO.get(shape, 0.0), ro)
        print(f"derive {_shape_id(shape)} {kind} sign={sign}: round-off {ro:.6g} (this shape so far: {_DERIVE_RO[shape]:.6g})")
        assert prof["launches"] == 1 and prof["blocks"] == n_digits * 6, prof
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{shape} {kind} sign={sign}: {len(bad)} limbs differ from the oracle, the first at (digit, index) {bad[0]}"
        old = got_digits(pkg.Address.set_from_fheuint(ram, fu, sign=sign))
        assert np.array_equal(got, old), f"{shape} {kind} sign={sign}: differs from fheram_address_set_from_fheuint (per-term inverse)"
        assert 0.0 < ro < PRECISION, (shape, kind, sign, ro)
    assert ram.roundoff_max(check=False) < PRECISION   # (the per-term path, on the same operands)


def test_eight_different_integers_in_one_launch_2_14(po):
    """K = 8 at 2^14, default plan: four of the kinds, a second draw of random signs and three integers whose bits are of different kinds.
    Each address against its own single derivation and the oracle: a fu[k] / out[k] mix-up cannot pass."""
    shape = DERIVE_SHAPES[0]
    w = derive_world(po, *shape)
    pkg, ram = w.pkg, w.ram
    # ("flipped" is not among them: it derives the very digits "lo" does — the oracle agrees — since 2^17 - 1 more at coefficient 0 of EVERY
    # operand polynomial adds the same (2^17 - 1) * x to every limb of a product, which the base-2^17 normalisation cancels limb against
    # limb; two integers with the same digits could be mixed up unseen, which the pairwise check below rules out)
    kinds = [k for k in KINDS if k != "flipped"] + ["signs2", "mixed0", "mixed1", "mixed3"]
    fus = [pkg.FheUintPrepared.from_host(ram, w.bits(k)) for k in kinds]
    singles = []
    for k, fu in zip(kinds, fus):
        a, = ram.derive_addresses([fu])
        singles.append(got_digits(a))
        assert np.array_equal(singles[-1], w.digits(k, False)), k
    for i in range(len(kinds)):
        for j in range(i):
            assert not np.array_equal(singles[i], singles[j]), (kinds[i], kinds[j])
    ram.roundoff_reset()
    ram.profile_enable(True)
    ram.profile_reset()
    addrs = ram.derive_addresses(fus)
    prof = ram.profile_get("derive")
    ram.profile_enable(False)
    ro = ram.roundoff_max(check=False)
    print(f"derive K=8 at 2^14: round-off {ro:.6g}")
    assert prof["launches"] == 1 and prof["blocks"] == 8 * 5 * 6, prof
    for k, a, s in zip(kinds, addrs, singles):
        got = got_digits(a)
        assert np.array_equal(got, s), f"{k}: the batched derivation differs from the single one"
        assert np.array_equal(got, w.digits(k, False)), k
    assert 0.0 < ro < PRECISION, ro


# =====================================================================================================================================
# B. the table forms at 2^16: 16 rows, coordinate 1 has two digits (base2d [[3,3,3,3],[3,1]])
# =====================================================================================================================================
MAX16 = 1 << 16
CONFIGS = [{"monitor": 2}, {"monitor": 2, "fuse": 0}]
_OPERANDS, _OCTX, _OFLOWS, _OREADS, _GKEYS = {}, {}, {}, {}, {}
_TABLE_RO = {"max": 0.0}


def params16(ws):
    return load_package().Parameters(max_addr=MAX16, word_size=ws)


def operand(role, kind, ws=0):
    """the limbs of one operand, the same wherever the kind is used again.  role: atk / atk_inv / tsk (keys), addr, rows, words"""
    key = (role, kind, ws)
    if key not in _OPERANDS:
        p = params16(max(ws, 1))
        shape = {"atk": (12, 3 * 4 * 2 * N), "atk_inv": (4 * 5 * 2 * N,), "tsk": (4 * 5 * 2 * N,), "addr": (p.base2d().as_1d().size(), p.ggsw_len()),
                 "rows": (ws, p.rows(), p.glwe_len()), "words": (ws, p.glwe_len())}[role]
        _OPERANDS[key] = _fill(kind, shape, _rng(*key))
    return _OPERANDS[key]


def gpu_keys(kind):
    if kind not in _GKEYS:
        pkg = load_package()
        _GKEYS[kind] = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(operand("atk", kind)), operand("atk_inv", kind), operand("tsk", kind))
    return _GKEYS[kind]


def octx(po, ws, keys_kind):
    if (ws, keys_kind) not in _OCTX:
        o = po.Oracle(po.OParams(max_addr=MAX16, word_size=ws)).set_threads(_threads())
        evk = {"gal_els": np.array([int(po.lib().fo_galois_element(12, i)) for i in range(12)], dtype=np.int64),
               "atk_glwe": operand("atk", keys_kind), "atk_ggsw_inv": operand("atk_inv", keys_kind), "tsk": operand("tsk", keys_kind)}
        _OCTX[(ws, keys_kind)] = (o, o.keys_prepare(evk))
    return _OCTX[(ws, keys_kind)]


def oracle_flow(po, ws, keys_kind, member):
    """the oracle's read, read_prepare_write, write and read-back of ONE member (rows, address digits, words: its kinds)"""
    key = (ws, keys_kind) + tuple(member)
    if key not in _OFLOWS:
        rows_k, addr_k, words_k = member
        o, okeys = octx(po, ws, keys_kind)
        o.reset_stats()
        addr = o.address_new(operand("addr", addr_k))
        ram = o.ram_new()
        ram.load(operand("rows", rows_k, ws))
        out = {"read": ram.read(addr, okeys), "rpw": ram.read_prepare_write(addr, okeys)}
        ram.write(operand("words", words_k, ws), addr, okeys)
        out["rows_after_write"] = ram.store()
        out["read_back"] = ram.read(addr, okeys)
        big = o.max_big()
        assert big < 1 << 47, (key, big)          # the bound the rounding contract is stated for
        _OFLOWS[key] = out
    return _OFLOWS[key]


def oracle_read(po, ws, keys_kind, rows_k, addr_k):
    key = (ws, keys_kind, rows_k, addr_k)
    if key not in _OREADS:
        o, okeys = octx(po, ws, keys_kind)
        o.reset_stats()
        ram = o.ram_new()
        ram.load(operand("rows", rows_k, ws))
        _OREADS[key] = ram.read(o.address_new(operand("addr", addr_k)), okeys)
        big = o.max_big()
        assert big < 1 << 47, (key, big)
    return _OREADS[key]


def note_roundoff(owner, what):
    ro = owner.roundoff_max(check=False)
    _TABLE_RO["max"] = max(_TABLE_RO["max"], ro)
    print(f"{what}: round-off through the table forms {ro:.6g} (this module so far: {_TABLE_RO['max']:.6g})")
    assert 0.0 < ro < PRECISION, (what, ro)


def first_difference(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else (len(bad), tuple(int(x) for x in bad[0]))


def bank_flow(po, keys_kind, members, ws, cfg):
    """read, read_prepare_write, write and read-back on the whole range of a bank whose member m holds rows, reads at an address and is
    written words of ITS kinds (members[m]); every result, the rows after the write and the read-back per member against the oracle's flow
    on that member; the launches each op took"""
    pkg = load_package()
    M, p = len(members), params16(ws)
    rows = p.rows()
    bank = pkg.RamBank(p, M, 0, config=cfg)
    keys = gpu_keys(keys_kind)
    for m, (rows_k, _, _) in enumerate(members):
        bank.load_encrypted(m, operand("rows", rows_k, ws))
    A = [pkg.Address(p, list(operand("addr", addr_k))) for _, addr_k, _ in members]
    W = np.stack([operand("words", words_k, ws) for _, _, words_k in members])
    bank._use_keys(keys)
    want = [oracle_flow(po, ws, keys_kind, mb) for mb in members]
    for i in range(M):   # no two members alike in anything: an operand, a row or a word taken from the wrong member shows
        for j in range(i):
            assert all(a != b for a, b in zip(members[i], members[j])) and {members[i][1], members[j][1]} != {"lo", "flipped"}, (i, j)
            assert not any(np.array_equal(want[i][k], want[j][k]) for k in want[i]), (i, j)
    t0, profs = bank.tail_stats(), {}

    def check(op, got):
        for m in range(M):
            assert first_difference(got[m], want[m][op]) is None, (keys_kind, members, cfg, op, "member", m, first_difference(got[m], want[m][op]))

    got, profs["read"] = profiled(bank, lambda: bank.read(A, keys), CLASSES)
    check("read", got)
    got, profs["rpw"] = profiled(bank, lambda: bank.read_prepare_write(A, keys), CLASSES)
    check("rpw", got)
    _, profs["write"] = profiled(bank, lambda: bank.write(W, A, keys), CLASSES)
    check("rows_after_write", [bank.store_encrypted(m) for m in range(M)])
    got, profs["read_back"] = profiled(bank, lambda: bank.read(A, keys), CLASSES)
    check("read_back", got)
    assert [bank.state(m) for m in range(M)] == [False] * M
    fused = cfg.get("fuse", 1) != 0
    for op, prof in profs.items():
        print(f"bank of {M} {cfg} {op}: " + ", ".join(f"{c} {v['launches']}x/{v['blocks']}" for c, v in prof.items() if v["launches"]))
        cls = "write_chain_launch" if op == "write" else "read_chain_launch"
        if fused:    # ONE table launch over the range, never one per member
            assert prof[cls]["launches"] == 1 and prof[cls]["blocks"] == rows * M * ws, (op, prof)
        else:        # (use_row_fuse needs the switch)
            assert prof[cls]["launches"] == 0, (op, prof)
        if op != "write":
            if M * ws <= 8:   # TAIL_GROUPS: coordinate 1's products and the trace as ONE k_trace_tail_t
                assert prof["keyswitch_tail_launch"]["launches"] == 1 and prof["keyswitch_mid_launch"]["launches"] == 0, (op, prof)
            else:             # the mid chain over the whole range
                assert prof["keyswitch_mid_launch"]["launches"] >= 1 and prof["keyswitch_tail_launch"]["launches"] == 0, (op, prof)
    t1, ms = bank.tail_stats(), bank.mid_stats()
    note_roundoff(bank, f"bank of {M}, keys {keys_kind}, members {members}, {cfg}")
    return t0, t1, ms


# B1: (kind of the keys, (rows, address digits, written words) of member 0, ... of member 1).  Rows, digits and words are of a different kind
# per member — the digits never "lo" against "flipped", which act alike as an operand (test_eight_different_integers_in_one_launch_2_14)
# — so that a launch that took member 1's digits, rows or words for member 0 cannot pass; bank_flow asserts that the members' expected
# results differ.  The members' kinds are those of PATTERNS[0], [1], [2], [4] and [5] where the rule allows, the keys one kind per case.
B1_CASES = [
    ("lo", (("lo", "lo", "lo"), ("flipped", "hi", "alternating"))),
    ("hi", (("hi", "hi", "hi"), ("alternating", "lo", "alternating"))),
    ("signs", (("signs", "signs", "signs"), ("lo", "hi", "hi"))),
    ("alternating", (("lo", "lo", "lo"), ("signs", "hi", "alternating"))),
]


def _case_id(c):
    return c[0] + "+" + "+".join("-".join(m) for m in c[1])


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
@pytest.mark.parametrize("case", B1_CASES, ids=_case_id)
def test_bank_of_two_members_of_different_kinds_2_16(po, case, cfg):
    """M = 2 at ws = 4: 8 ciphertexts, so each op is ONE k_read_chain_t / k_write_chain_t over both members and the end of a read ONE
    k_trace_tail_t, which does not give up"""
    keys_kind, members = case
    t0, t1, _ = bank_flow(po, keys_kind, members, 4, cfg)
    assert t1["launches"] == t0["launches"] + 3 and t1["fallbacks"] == t0["fallbacks"], (t0, t1)


def test_tail_fallback_sees_extreme_operands_2_16(po):
    """tail_test: every k_trace_tail_t gives up late, and the predicated k_read_chain_t behind it redoes coordinate 1's products (digits of
    member y / ws) and the trace"""
    keys_kind, members = B1_CASES[3]
    t0, t1, _ = bank_flow(po, keys_kind, members, 4, {"monitor": 2, "tail_test": 1})
    assert t1["launches"] == t0["launches"] + 3 and t1["fallbacks"] == t0["fallbacks"] + 3, (t0, t1)


# B2: a third member behind those of a B1 case: 12 ciphertexts
B2_CASES = [
    ("lo", B1_CASES[0][1] + (("signs", "alternating", "hi"),)),
    ("hi", B1_CASES[1][1] + (("lo", "signs", "lo"),)),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
@pytest.mark.parametrize("case", B2_CASES, ids=_case_id)
def test_bank_of_three_members_ends_in_the_mid_chain_2_16(po, case, cfg):
    keys_kind, members = case
    t0, t1, ms = bank_flow(po, keys_kind, members, 4, cfg)
    assert t1["launches"] == t0["launches"], (t0, t1)
    assert ms["launches"] > 0 and ms["fallbacks"] == 0, ms


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
def test_read_batch_of_four_kinds_of_address_2_16(po, cfg):
    """K = 4 at ws = 2 on one RAM: 8 ciphertexts, the end of the batch is ONE k_trace_tail_t with the digits of address y / ws"""
    pkg = load_package()
    ws, keys_kind, rows_k, addr_ks = 2, "signs", "alternating", ["lo", "hi", "alternating", "signs"]
    p = params16(ws)
    ram = pkg.Ram(p, 0, config=cfg)
    ram.load_encrypted(operand("rows", rows_k, ws))
    keys = gpu_keys(keys_kind)
    ram._use_keys(keys)
    A = [pkg.Address(p, list(operand("addr", k))) for k in addr_ks]
    want = [oracle_read(po, ws, keys_kind, rows_k, k) for k in addr_ks]
    t0 = ram.tail_stats()
    ram.profile_enable(True)
    ram.profile_reset()
    got = ram.read_batch(A, keys)
    prof = {c: ram.profile_get(c) for c in CLASSES}
    ram.profile_enable(False)
    print(f"read_batch K=4 ws=2 {cfg}: " + ", ".join(f"{c} {v['launches']}x/{v['blocks']}" for c, v in prof.items() if v["launches"]))
    for k in range(4):
        assert first_difference(got[k], want[k]) is None, (cfg, "address", k, addr_ks[k], first_difference(got[k], want[k]))
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(want[i], want[j]), (i, j)
    assert prof["keyswitch_tail_launch"]["launches"] == 1, prof
    t1 = ram.tail_stats()
    assert t1["launches"] == t0["launches"] + 1 and t1["fallbacks"] == t0["fallbacks"], (t0, t1)
    assert np.array_equal(ram.store_encrypted(), operand("rows", rows_k, ws)) and not ram.state
    note_roundoff(ram, f"read_batch of {addr_ks}, {cfg}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=["default", "fuse0"])
def test_read_list_over_members_of_different_kinds_2_16(po, cfg):
    """[0, 0, 1, 2] on a 3-member bank at ws = 2: 8 ciphertexts through ONE k_read_chain_t whose source map is neither all 0 nor the
    identity, and ONE k_trace_tail_t; every entry against the oracle's read of THAT member at THAT address"""
    pkg = load_package()
    ws, keys_kind = 2, "signs"
    member_rows = ["lo", "signs", "alternating"]
    members, addr_ks = [0, 0, 1, 2], ["hi", "signs", "lo", "alternating"]
    p = params16(ws)
    rows = p.rows()
    bank = pkg.RamBank(p, 3, 0, config=cfg)
    for m, k in enumerate(member_rows):
        bank.load_encrypted(m, operand("rows", k, ws))
    keys = gpu_keys(keys_kind)
    bank._use_keys(keys)
    A = [pkg.Address(p, list(operand("addr", k))) for k in addr_ks]
    want = [oracle_read(po, ws, keys_kind, member_rows[m], k) for m, k in zip(members, addr_ks)]
    for i in range(4):
        for j in range(i):
            assert not np.array_equal(want[i], want[j]), (i, j)
    snaps = [member_snapshot(bank, m) for m in range(3)]
    t0 = bank.tail_stats()
    got, prof = profiled(bank, lambda: bank.read_list(members, A, keys), CLASSES)
    print(f"read_list {members} ws=2 {cfg}: " + ", ".join(f"{c} {v['launches']}x/{v['blocks']}" for c, v in prof.items() if v["launches"]))
    for k, m in enumerate(members):
        assert first_difference(got[k], want[k]) is None, (cfg, "entry", k, "member", m, addr_ks[k], first_difference(got[k], want[k]))
    for m in range(3):   # a read changes no member: rows, tree level 0 and state are where they were
        assert_member_is(bank, m, snaps[m], "after the list")
        assert np.array_equal(snaps[m][0], operand("rows", member_rows[m], ws)) and snaps[m][2] is False
    if cfg.get("fuse", 1):
        assert prof["read_chain_launch"]["launches"] == 1 and prof["read_chain_launch"]["blocks"] == rows * 4 * ws, prof
    else:
        assert prof["read_chain_launch"]["launches"] == 0, prof
    assert prof["keyswitch_tail_launch"]["launches"] == 1 and prof["keyswitch_mid_launch"]["launches"] == 0, prof
    t1 = bank.tail_stats()
    assert t1["launches"] == t0["launches"] + 1 and t1["fallbacks"] == t0["fallbacks"], (t0, t1)
    note_roundoff(bank, f"read_list {members} of {member_rows} at {addr_ks}, {cfg}")
