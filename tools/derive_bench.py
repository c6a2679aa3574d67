#!/usr/bin/env python3
"""Addresses from encrypted integers: fheram_address_derive (one launch for K integers, into existing addresses) against K calls of the
unchanged fheram_address_set_from_fheuint (four launches per bit and digit, allocations, a host wait each).

Legs per K (one GPU, one context, both legs in this tree's library: the old entry point and its kernels are untouched):
  old     K calls of Address.set_from_fheuint, then fheram_sync                                  (baseline a)
  derive  one Ram.derive_addresses of K integers into K existing addresses, then fheram_sync     (candidate b)
The addresses the old leg creates are kept until the clock has stopped (freeing them is not charged to it).
Also, at K = 2 on a 2-member bank: derive + bank read + sync against the derive alone and the read alone.

Method as tools/bank_bench.py: host clock around calls that end in a sync, the legs alternated repetition by repetition, the median of
--reps repetitions, the p10..p90 spread of the baseline.  Inputs are synthetic normalised limbs from fixed seeds (as bench.py's); the two
legs' digits are compared once per K.  The round-off monitor's maximum after the derivations is recorded next to the times (the 8-term
accumulation of k_cmux_chain is the widest sum on any path).

Acceptance: derive beats old per address by more than old's spread.

  python tools/derive_bench.py --log-max-addr 14 --out profiles/derive_2p14.json
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


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def summarise(xs):
    med = float(np.median(xs))
    return {"median_ms": med * 1e3, "min_ms": min(xs) * 1e3, "max_ms": max(xs) * 1e3, "p10_ms": pct(xs, 10) * 1e3, "p90_ms": pct(xs, 90) * 1e3,
            "spread_rel": (pct(xs, 90) - pct(xs, 10)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-max-addr", type=int, default=14)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--word-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from _pkg import load_package
    pkg = load_package()
    p = pkg.Parameters(max_addr=1 << args.log_max_addr, word_size=args.word_size)
    n_bits = args.log_max_addr
    n_digits = p.base2d().as_1d().size()
    ram = pkg.Ram(p, 0)
    fu_len = pkg.library().fheram_fheuint_ggsw_len(ram._h)
    rng = np.random.default_rng(2718)
    kmax = max(int(x) for x in args.ks.split(","))
    bits = [synth(rng, (n_bits, fu_len)) for _ in range(kmax)]
    fus = [pkg.FheUintPrepared.from_host(ram, b) for b in bits]
    result = {"tool": "tools/derive_bench.py", "log_max_addr": args.log_max_addr, "n_digits": n_digits, "reps": args.reps,
              "clock": "host perf_counter around calls that end in fheram_sync", "spread": "p10..p90 of the repetitions of a leg over its median",
              "device": ram.device_info(), "old_launches_per_address": 4 * n_bits, "k": {}}

    def leg_old(K):
        t0 = time.perf_counter()
        made = [pkg.Address.set_from_fheuint(ram, fus[i], sign=False) for i in range(K)]
        ram.sync()
        return time.perf_counter() - t0, made

    for K in [int(x) for x in args.ks.split(",")]:
        addrs = [pkg.Address.alloc(ram) for _ in range(K)]

        def leg_new():
            t0 = time.perf_counter()
            ram.derive_addresses(fus[:K], addrs)
            ram.sync()
            return time.perf_counter() - t0

        ram.roundoff_reset()
        _, made = leg_old(K)
        leg_new()
        same = all(np.array_equal(np.stack(a.digits), np.stack(b.digits)) for a, b in zip(made, addrs))
        for a in addrs:
            a._digits = None
        del made
        for _ in range(args.warmup):
            leg_old(K)
            leg_new()
        t = {"old": [], "derive": []}
        for _ in range(args.reps):            # alternating: one repetition of each leg in turn
            dt, made = leg_old(K)
            t["old"].append(dt)
            del made
            t["derive"].append(leg_new())
        ram.profile_enable(True)
        ram.profile_reset()
        leg_new()
        prof = ram.profile_get("derive")
        ram.profile_enable(False)
        s = {k: summarise(v) for k, v in t.items()}
        gain = s["old"]["median_ms"] / s["derive"]["median_ms"]
        entry = {"digits_equal_to_old_entry_point": bool(same), "per_call_of_K_addresses": s,
                 "ms_per_address": {k: s[k]["median_ms"] / K for k in s}, "baseline_spread_rel": s["old"]["spread_rel"],
                 "derive_speedup_over_old": gain, "accept_beats_old_by_more_than_spread": bool(gain > 1.0 + s["old"]["spread_rel"]),
                 "launch_profile": {"class": "derive", "launches": prof["launches"], "blocks": prof["blocks"], "device_ms": prof["ms"]},
                 "roundoff_max_after_derivations": ram.roundoff_max(check=False)}
        result["k"][str(K)] = entry
        print(f"2^{args.log_max_addr} K={K}: old {s['old']['median_ms']:.3f} ms  derive {s['derive']['median_ms']:.3f} ms  gain {gain:.2f}  "
              f"old spread {s['old']['spread_rel']:.3f}  equal {same}  round-off {entry['roundoff_max_after_derivations']:.3g}", flush=True)

    # a 2-member bank: the derive in front of the read it feeds
    bank = pkg.RamBank(p, 2, 0)
    rng = np.random.default_rng(1234)
    keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
    for m in range(2):
        bank.load_encrypted(m, synth(rng, (args.word_size, p.rows(), p.glwe_len())))
    bank._use_keys(keys)
    bfus = [pkg.FheUintPrepared.from_host(bank, b) for b in bits[:2]]
    baddrs = bank.derive_addresses(bfus)
    bank.sync()

    def b_derive():
        bank.derive_addresses(bfus, baddrs)

    def b_read():
        bank.read(baddrs, keys, download=False)

    legs = {"derive": (b_derive,), "read": (b_read,), "derive_then_read": (b_derive, b_read)}
    tb = {k: [] for k in legs}
    for rep in range(args.warmup + args.reps):
        for name, fns in legs.items():
            t0 = time.perf_counter()
            for f in fns:
                f()
            bank.sync()
            if rep >= args.warmup:
                tb[name].append(time.perf_counter() - t0)
    sb = {k: summarise(v) for k, v in tb.items()}
    result["bank_m2_k2"] = {"legs": sb, "sum_of_parts_ms": sb["derive"]["median_ms"] + sb["read"]["median_ms"],
                            "roundoff_max": bank.roundoff_max(check=False)}
    print(f"2^{args.log_max_addr} bank M=2 K=2: derive {sb['derive']['median_ms']:.3f} ms  read {sb['read']['median_ms']:.3f} ms  "
          f"derive+read {sb['derive_then_read']['median_ms']:.3f} ms", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
