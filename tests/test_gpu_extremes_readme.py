"""Extreme limbs through the 5-limb instantiations: tests/test_gpu_extremes.py feeds limbs at the ends of the normalised range through the
<4, 4> chain kernels only.  Here the same flow (read, read_prepare_write, write, rows, read back) runs on the README block (k_evk_trace = 85,
k_glwe_pt = 9: trace keys of shape (12, 3 * 5 * 2 * N)), where the sums are as large — with 5-limb keys the oracle's largest accumulator is
still 6 * 4096 * 2^32 = 2^46.585, below the 2^47 the rounding contract is stated for (asserted on every case) — and the limb loops, LDS and
register footprints are those of k_read_chain<5,4>, k_write_chain<5,4>, k_keyswitch_chain<3,5,3>, k_trace_tail<3,5,3> and k_chain_mid<.,5,.,.>.

Sizes.  launch.hpp chain_form puts a chain of `batch` ciphertexts in the Chain form (one workgroup per ciphertext: k_read_chain / k_write_chain
through use_row_fuse) only when pick_nco says 2, i.e. batch * 2 > 256 CUs: batch >= 129.  At word_size 2 that is 65 rows, so the SMALLEST
max_addr whose profiled read and write show read_chain_launch / write_chain_launch is 64 * 4096 + 1 = 262145 (130 ciphertext rows; the last row
holds one word).  Up to 48 ciphertexts (5-limb keys) a trace chain is in the Mid form; 2^14 at word_size 4 is 16 ciphertext rows, k_chain_mid
for the products and for the alone levels (at word_size 2 it would be 8 ciphertext rows, the Tail form, which the larger size ends in anyway).
The classes are asserted from the launch profile of the default configuration.

Round-off (fheram_roundoff_max under monitor = 2, every coefficient watched; 3/8 is the library's contract and raises above it).  Every case
prints its maximum; measured on an MI355X they are, the same in all three configurations:
    pattern                          65 rows x 2    2^14 x 4
    hi-hi-hi-hi                      0.1562         0.0703
    alternating-lo-hi-alternating    0.0391         0.0391
    flipped-lo-lo-flipped            0.1094         0.0469
    signs-signs-signs-signs          0.0024         0.0016
    the mix top: hi 0.0391, alternating 0.0195
None is above the 0.25 the 4-limb test asserts (its own largest is 0.156 too), so 0.25 is asserted here as well.
The inputs are not ciphertexts: nothing decrypts, everything compares."""
import zlib

import numpy as np
import pytest

from _pkg import load_package
from test_gpu_extremes import N, _fill, _threads

pytestmark = pytest.mark.gpu
README = {"k_glwe_pt": 9, "k_evk_trace": 85}
ROUNDOFF = 0.25   # what tests/test_gpu_extremes.py asserts for the 4-limb kernels; every measured maximum is below it (module docstring)
SMALLEST_CHAIN = 64 * N + 1   # 65 rows x word_size 2 = 130 > 128 ciphertext rows (module docstring)
CLASSES = ["read_chain_launch", "write_chain_launch", "keyswitch_mid_launch", "ext_product_mid_launch", "keyswitch_tail_launch"]
# (kind of the rows, of the address digits, of the keys, of the written words)
PATTERNS = [("hi", "hi", "hi", "hi"), ("alternating", "lo", "hi", "alternating"), ("flipped", "lo", "lo", "flipped"), ("signs", "signs", "signs", "signs")]


def gal_els(po):
    return np.array([int(po.lib().fo_galois_element(12, i)) for i in range(12)], dtype=np.int64)


def keys_of(kind, rng):
    return {"atk": _fill(kind, (12, 3 * 5 * 2 * N), rng), "atk_inv": _fill(kind, 4 * 5 * 2 * N, rng), "tsk": _fill(kind, 4 * 5 * 2 * N, rng)}


def okeys_of(po, o, inp):
    return o.keys_prepare({"gal_els": gal_els(po), "atk_glwe": inp["atk"], "atk_ggsw_inv": inp["atk_inv"], "tsk": inp["tsk"]})


def oracle_flow(po, max_addr, ws, inp):
    o = po.Oracle(po.OParams(max_addr=max_addr, word_size=ws, **README)).set_threads(_threads())
    keys = okeys_of(po, o, inp)
    addr = o.address_new(inp["addr"])
    ram = o.ram_new()
    ram.load(np.ascontiguousarray(inp["rows"]))
    out = {"read": ram.read(addr, keys), "rpw": ram.read_prepare_write(addr, keys)}
    ram.write(np.ascontiguousarray(inp["words"]), addr, keys)
    out["rows_after_write"] = ram.store()
    out["read_back"] = ram.read(addr, keys)
    assert o.max_big() < 1 << 47          # the bound the rounding contract is stated for
    return out


def profiled(ram, fn):
    ram.profile_enable(True)
    ram.profile_reset()
    out = fn()
    ram.sync()
    prof = {c: ram.profile_get(c)["launches"] for c in CLASSES}
    ram.profile_enable(False)
    return out, prof


@pytest.mark.parametrize("max_addr,ws", [(SMALLEST_CHAIN, 2), (1 << 14, 4)], ids=["65rows_x2", "2p14_x4"])
@pytest.mark.parametrize("pat", PATTERNS, ids=lambda p: "-".join(p))
def test_extreme_limbs_through_the_5_limb_chain_kernels(po, pat, max_addr, ws):
    """the flow of test_extreme_limbs_through_the_chain_kernels under 5-limb trace keys, in the default configuration and in the limb-form
    (chain_y = 0) and unfused (fuse = 0) chains.  Measured round-off maxima: 0.0016 .. 0.1562 (the module docstring's table); asserted <= 0.25."""
    pkg = load_package()
    rng = np.random.default_rng(zlib.crc32(("readme-" + "-".join(pat)).encode()))
    p = pkg.Parameters(max_addr=max_addr, decomp_n=[3, 3, 3, 3], word_size=ws, **README)
    n_digits = p.base2d().as_1d().size()
    rows_r, addr_r, keys_r, words_r = pat
    inp = dict(keys_of(keys_r, rng), addr=_fill(addr_r, (n_digits, p.ggsw_len()), rng), rows=_fill(rows_r, (ws, p.rows(), p.glwe_len()), rng),
               words=_fill(words_r, (ws, p.glwe_len()), rng))
    want = oracle_flow(po, max_addr, ws, inp)
    worst = 0.0
    for cfg in ({"monitor": 2}, {"monitor": 2, "chain_y": 0}, {"monitor": 2, "fuse": 0}):
        ram = pkg.Ram(p, config=cfg)
        keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(inp["atk"]), inp["atk_inv"], inp["tsk"])
        addr = pkg.Address(p, list(inp["addr"]))
        ram.load_encrypted(inp["rows"])
        ram._use_keys(keys)
        default = len(cfg) == 1
        run = profiled if default else (lambda r, fn: (fn(), None))
        got = {}
        got["read"], prof_read = run(ram, lambda: ram.read(addr, keys).copy())
        got["rpw"] = ram.read_prepare_write(addr, keys)
        _, prof_write = run(ram, lambda: ram.write(inp["words"], addr, keys))
        got["rows_after_write"] = ram.store_encrypted()
        got["read_back"] = ram.read(addr, keys)
        for k in ("read", "rpw", "rows_after_write", "read_back"):
            bad = np.count_nonzero(np.asarray(got[k]).ravel() != np.asarray(want[k]).ravel())
            assert bad == 0, (pat, cfg, k, bad)
        if default and max_addr == SMALLEST_CHAIN:   # k_read_chain<5,4> / k_write_chain<5,4>, and the tail the read ends in (k_trace_tail<3,5,3>)
            assert prof_read["read_chain_launch"] == 1 and prof_read["keyswitch_mid_launch"] == 0 and prof_read["ext_product_mid_launch"] == 0, prof_read
            assert prof_read["keyswitch_tail_launch"] >= 1, prof_read
            assert prof_write["write_chain_launch"] == 1 and prof_write["keyswitch_mid_launch"] == 0 and prof_write["ext_product_mid_launch"] == 0, prof_write
        elif default:                               # k_chain_mid<true,4,3,2> for the products, k_chain_mid<false,5,3,2> for the trace chains
            assert prof_read["read_chain_launch"] == 0 and prof_read["ext_product_mid_launch"] >= 1 and prof_read["keyswitch_mid_launch"] >= 1, prof_read
            assert prof_write["write_chain_launch"] == 0 and prof_write["keyswitch_mid_launch"] >= 1, prof_write
        ro = ram.roundoff_max()              # the library's own contract: raises FHERAM_ERR_PRECISION above 3/8
        print(f"extremes readme {'-'.join(pat)} max_addr={max_addr} x{ws} {cfg}: round-off maximum {ro:.4g}")
        assert 0.0 < ro <= ROUNDOFF, (pat, cfg, ro)
        worst = max(worst, ro)
        assert ram.tail_stats()["fallbacks"] == 0
        del ram
    print(f"extremes readme {'-'.join(pat)} max_addr={max_addr} x{ws}: max round-off through the chains {worst:.4g}")


@pytest.mark.parametrize("kind", ["hi", "alternating"])
def test_extreme_limbs_through_the_mix_top(po, kind):
    """2^12, word_size 2: ONE read_mix of a member row, a 12-bit table row and a 5-bit register row whose every polynomial — rows, address
    digits, selector digits, keys — is the pattern; equal to the oracle's Ram::read of the three RAMs, under monitor = 2
    (k_trace_tail_x<3,5,3>: one keyswitch_tail_launch, no fallback).  Measured round-off maxima: hi 0.0391, alternating 0.0195; asserted <= 0.25."""
    pkg = load_package()
    ws = 2
    rng = np.random.default_rng(zlib.crc32(("readme-mix-" + kind).encode()))
    p = pkg.Parameters(max_addr=1 << 12, word_size=ws, **README)
    inp = keys_of(kind, rng)
    G, GG = p.glwe_len(), p.ggsw_len()
    rows = {"member": _fill(kind, (ws, 1, G), rng), "table": _fill(kind, (ws, 1, G), rng), "regs": _fill(kind, (ws, 1, G), rng)}
    digits = {"member": _fill(kind, (4, GG), rng), "table": _fill(kind, (4, GG), rng), "regs": _fill(kind, (2, GG), rng)}
    want = {}
    for what, max_addr in (("member", 1 << 12), ("table", 1 << 12), ("regs", 1 << 5)):
        o = po.Oracle(po.OParams(max_addr=max_addr, word_size=ws, **README)).set_threads(_threads())
        assert o.n_digits == digits[what].shape[0]
        oram = o.ram_new()
        oram.load(np.ascontiguousarray(rows[what]))
        want[what] = oram.read(o.address_new(digits[what]), okeys_of(po, o, inp))
        assert o.max_big() < 1 << 47
    bank = pkg.RamBank(p, 1, 0, config={"monitor": 2})
    bank._use_keys(pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(inp["atk"]), inp["atk_inv"], inp["tsk"]))
    bank.load_encrypted(0, rows["member"])
    t, rf = bank.table(12), bank.regfile(5)
    t.load(rows["table"].reshape(ws, -1))
    rf.load(rows["regs"].reshape(ws, -1))
    addr = pkg.Address(p, list(digits["member"]))
    tsel = bank.table_selector(12, list(digits["table"]))
    rsel = pkg.Selector.from_digits(bank, 5, list(digits["regs"]))
    f0 = bank.tail_stats()["fallbacks"]
    bank.profile_enable(True)
    bank.profile_reset()
    got = bank.read_mix(([0], [addr]), ([t], [tsel]), (rf, [rsel]))
    bank.sync()
    launches = bank.profile_get("keyswitch_tail_launch")["launches"]
    bank.profile_enable(False)
    for g, what in zip(got, ("member", "table", "regs")):
        bad = np.count_nonzero(np.asarray(g[0]).ravel() != np.asarray(want[what]).ravel())
        assert bad == 0, (kind, what, bad)
    assert launches == 1 and bank.tail_stats()["fallbacks"] == f0, (launches, bank.tail_stats())
    ro = bank.roundoff_max()
    print(f"extremes readme mix top {kind}: round-off maximum {ro:.4g}")
    assert 0.0 < ro <= ROUNDOFF, (kind, ro)

