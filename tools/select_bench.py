#!/usr/bin/env python3
"""The conditional-write step of a VM on two members of a bank — `enable ? new : old`, the opcode encrypted — with the select on the device
(fheram_bank_select / fheram_bank_write_list_selected) against the only route the entry points before it offer.

Legs (one GPU, a bank of three members, the step on members {0, 2}; both legs in this tree's library, leg (a) through the older entry points only):
  host    (a) read_prepare_write_list with download; the pack old + X * new in numpy; upload into a helper bank of max_addr = 2^1 (two members);
              derive the helper's addresses from the enable integers; helper read with download; write_list with those host words; sync
  device  (b) read_prepare_write_list(out = NULL); selector_derive; select(out = NULL); write_list_selected; one sync
Also: the select alone (n = 1, two candidates, then sync) beside a single-member fheram_bank_read at 2^12 (the same chain without the pack),
with the device time of the pack launch from the launch profile.

Method as tools/derive_bench.py: host clock around calls that end in a sync, the legs alternated repetition by repetition, the median of --reps
repetitions, the p10..p90 spread of the baseline.  Inputs are synthetic normalised limbs from fixed seeds (as bench.py's).

Acceptance: device beats host by more than host's spread.

  python tools/select_bench.py --log-max-addr 14 --out profiles/select_2p14.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 4096
MEMBERS = [0, 2]


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def summarise(xs):
    med = float(np.median(xs))
    return {"median_ms": med * 1e3, "min_ms": min(xs) * 1e3, "max_ms": max(xs) * 1e3, "p10_ms": pct(xs, 10) * 1e3, "p90_ms": pct(xs, 90) * 1e3,
            "spread_rel": (pct(xs, 90) - pct(xs, 10)) / med}


def host_pack(old, new):
    """glwe_normalize(old + X * new) on [.., 3 limbs, 2 columns, N] int64: the negacyclic shift by one, then one carry pass from the last limb"""
    s = old + np.concatenate([-new[..., -1:], new[..., :-1]], axis=-1)
    out = np.empty_like(s)
    carry = np.zeros(s.shape[:-3] + s.shape[-2:], dtype=np.int64)
    for limb in (2, 1, 0):
        v = s[..., limb, :, :] + carry
        carry = (v + (1 << 16)) >> 17
        out[..., limb, :, :] = v - (carry << 17)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-max-addr", type=int, default=14)
    ap.add_argument("--word-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from _pkg import load_package
    pkg = load_package()
    S = pkg.Src
    ws = args.word_size
    p = pkg.Parameters(max_addr=1 << args.log_max_addr, word_size=ws)
    rng = np.random.default_rng(1234)
    keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
    bank = pkg.RamBank(p, 3, 0)
    for m in range(3):
        bank.load_encrypted(m, synth(rng, (ws, p.rows(), p.glwe_len())))
    bank._use_keys(keys)
    fu_len = pkg.library().fheram_fheuint_ggsw_len(None)
    n_bits = max(args.log_max_addr, 2)
    bits = [synth(rng, (n_bits, fu_len)) for _ in range(4)]
    fus = [pkg.FheUintPrepared.from_host(bank, b) for b in bits]
    addrs = bank.derive_addresses(fus[:2])
    new = synth(rng, (2, ws, p.glwe_len()))
    sels = [bank.selector(1), bank.selector(1)]
    # leg (a)'s helper: a bank of two one-row RAMs of max_addr = 2, the same keys
    hp = pkg.Parameters(max_addr=2, word_size=ws)
    helper = pkg.RamBank(hp, 2, 0)
    helper._use_keys(keys)
    hfus = [pkg.FheUintPrepared.from_host(helper, b) for b in bits[2:]]
    haddrs = [pkg.Address.alloc(helper) for _ in range(2)]
    bank.sync()
    helper.sync()
    shape5 = (2, ws, 3, 2, N)

    def leg_host():
        t0 = time.perf_counter()
        old = bank.read_prepare_write_list(MEMBERS, addrs, keys)
        packed = host_pack(old.reshape(shape5), new.reshape(shape5)).reshape(2, ws, 1, -1)
        for m in range(2):
            helper.load_encrypted(m, packed[m])
        helper.derive_addresses(hfus, haddrs)
        words = helper.read(haddrs, keys)
        bank.write_list(MEMBERS, words, addrs, keys)
        bank.sync()
        return time.perf_counter() - t0

    def leg_device():
        t0 = time.perf_counter()
        bank.read_prepare_write_list(MEMBERS, addrs, keys, download=False)
        bank.derive_selectors(fus[2:], [0, 0], sels)
        bank.select(sels, [[S.member(0), S.host(0)], [S.member(2), S.host(1)]], host_words=new, download=False)
        bank.write_list_selected(MEMBERS, [0, 1], addrs, keys)
        bank.sync()
        return time.perf_counter() - t0

    result = {"tool": "tools/select_bench.py", "log_max_addr": args.log_max_addr, "word_size": ws, "members": MEMBERS, "reps": args.reps,
              "clock": "host perf_counter around calls that end in a sync", "spread": "p10..p90 of the repetitions of a leg over its median"}
    for _ in range(args.warmup):
        leg_host()
        leg_device()
    t = {"host": [], "device": []}
    for _ in range(args.reps):   # alternating: one repetition of each leg in turn
        t["host"].append(leg_host())
        t["device"].append(leg_device())
    s = {k: summarise(v) for k, v in t.items()}
    gain = s["host"]["median_ms"] / s["device"]["median_ms"]
    result["conditional_write_step"] = {"legs": s, "baseline_spread_rel": s["host"]["spread_rel"], "device_speedup_over_host": gain,
                                        "accept_beats_host_by_more_than_spread": bool(gain > 1.0 + s["host"]["spread_rel"])}
    bank.profile_enable(True)
    bank.profile_reset()
    leg_device()
    result["conditional_write_step"]["launch_profile_device_leg"] = {c: bank.profile_get(c) for c in ("select_pack", "derive", "prepare", "ext_product", "keyswitch", "elementwise")}
    bank.profile_enable(False)
    result["roundoff_max"] = bank.roundoff_max(check=False)
    print(f"2^{args.log_max_addr} conditional write on {MEMBERS}: host {s['host']['median_ms']:.3f} ms  device {s['device']['median_ms']:.3f} ms  gain {gain:.2f}  "
          f"host spread {s['host']['spread_rel']:.3f}", flush=True)

    # the select alone beside a read at 2^12: the same chain without the pack
    p12 = pkg.Parameters(max_addr=1 << 12, word_size=ws)
    one = pkg.RamBank(p12, 1, 0)
    one.load_encrypted(0, synth(rng, (ws, 1, p12.glwe_len())))
    one._use_keys(keys)
    fu12 = pkg.FheUintPrepared.from_host(one, bits[0][:12])
    a12 = one.derive_addresses([fu12])
    sel12 = one.selector(1)
    one.derive_selectors([fu12], [0], [sel12])
    one.sync()

    def t_read():
        t0 = time.perf_counter()
        one.read(a12, keys, download=False)
        one.sync()
        return time.perf_counter() - t0

    def t_select():
        t0 = time.perf_counter()
        one.select([sel12], [[S.host(0), S.host(1)]], host_words=new, download=False)
        one.sync()
        return time.perf_counter() - t0

    ts = {"read_2p12": [], "select_m2": []}
    for rep in range(args.warmup + args.reps):
        a, b = t_read(), t_select()
        if rep >= args.warmup:
            ts["read_2p12"].append(a)
            ts["select_m2"].append(b)
    one.profile_enable(True)
    one.profile_reset()
    for _ in range(10):
        t_select()
    pack = one.profile_get("select_pack")
    one.profile_enable(False)
    result["select_alone"] = {"legs": {k: summarise(v) for k, v in ts.items()},
                              "select_pack_device_us_per_launch": pack["ms"] * 1e3 / max(pack["launches"], 1), "select_pack_launches": pack["launches"],
                              "note": "the select stages two host candidates and multiplies by ONE digit; the read at 2^12 multiplies by the four digits of its coordinate"}
    r = result["select_alone"]["legs"]
    print(f"select alone {r['select_m2']['median_ms']:.3f} ms  read at 2^12 {r['read_2p12']['median_ms']:.3f} ms  pack {result['select_alone']['select_pack_device_us_per_launch']:.1f} us", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
