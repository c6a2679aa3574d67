#!/usr/bin/env python3
"""Latency of a step — read_prepare_write + write — on any set of members of a bank: the two list calls against what a host could do
before them.

Legs (per list, one bank of M members, one GPU; every leg ends in fheram_bank_sync):
  singles  per entry, a single-member fheram_bank_read_prepare_write; then per entry a single-member fheram_bank_write   (baseline a)
  ranges   the fewest contiguous ascending ranges that cover the list in entry order, a fheram_bank_read_prepare_write per
           range, then a fheram_bank_write per range: [0,2] and [1,0] are two ranges of one member, [2,1,0] three            (baseline b)
  list     fheram_bank_read_prepare_write_list + fheram_bank_write_list                                                      (candidate)
The baseline legs run code paths the lists leave alone (the contiguous-range operations and their kernels), on the same bank in the same
process, so they are the parent's numbers measured in the same session.  The legs alternate repetition by repetition.  Inputs are
synthetic normalised limbs from fixed seeds (as bench.py's).  Every timed list is compared once with its single operations (int64:
results and the rows of every member afterwards, on a second bank that runs the single operations).

Reported per list: the median of --reps repetitions of every leg (host clock around calls that end in a sync), the spread of the
better baseline (p10..p90 of its repetitions over its median), the verdict of the acceptance rule of DESIGN.md 10 — the list beats
the better baseline by more than that baseline's spread — and the launch profile of one further step.

  python tools/write_list_bench.py --log-max-addr 18 --out profiles/write_list_2p18.json
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
CLASSES = ["prepare", "read_chain_launch", "write_chain_launch", "ext_product", "keyswitch", "keyswitch_tail_launch", "keyswitch_mid_launch", "elementwise"]


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


def cover(members):
    """the fewest contiguous ascending runs, in entry order: [(first entry, first member, n)]"""
    runs, k = [], 0
    while k < len(members):
        e = k + 1
        while e < len(members) and members[e] == members[e - 1] + 1:
            e += 1
        runs.append((k, members[k], e - k))
        k = e
    return runs


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def summarise(xs):
    med = float(np.median(xs))
    return {"median_ms": med * 1e3, "min_ms": min(xs) * 1e3, "max_ms": max(xs) * 1e3, "p10_ms": pct(xs, 10) * 1e3, "p90_ms": pct(xs, 90) * 1e3,
            "spread_rel": (pct(xs, 90) - pct(xs, 10)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-max-addr", type=int, default=18)
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--word-size", type=int, default=4)
    ap.add_argument("--lists", default="0,2;2,1,0;1,0")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--iters", type=int, default=4, help="units per timed repetition")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from _pkg import load_package
    pkg = load_package()
    M, ws = args.members, args.word_size
    p = pkg.Parameters(max_addr=1 << args.log_max_addr, word_size=ws)
    rng = np.random.default_rng(1234)
    keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
    n_digits = p.base2d().as_1d().size()
    rng = np.random.default_rng(4321)
    addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(M)]
    words = synth(rng, (M, ws, p.glwe_len()))
    bank, twin = pkg.RamBank(p, M), pkg.RamBank(p, M)   # twin: the single operations the lists are compared with
    for m in range(M):
        rows = synth(rng, (ws, p.rows(), p.glwe_len()))
        bank.load_encrypted(m, rows)
        twin.load_encrypted(m, rows)
    bank._use_keys(keys)
    twin._use_keys(keys)
    result = {"tool": "tools/write_list_bench.py", "log_max_addr": args.log_max_addr, "members": M, "word_size": ws, "reps": args.reps,
              "iters_per_rep": args.iters, "clock": "host perf_counter around calls that end in fheram_bank_sync",
              "spread": "p10..p90 of the repetitions of the better baseline leg over its median", "lib": os.path.relpath(pkg.library_path(), ROOT),
              "lists": {}}

    for spec in args.lists.split(";"):
        members = [int(x) for x in spec.split(",")]
        A = [addrs[k] for k in range(len(members))]   # entry k at address k
        W = words[:len(members)]
        runs = cover(members)

        def singles():
            for k, m in enumerate(members):
                bank.read_prepare_write([A[k]], keys, first=m, download=False)
            for k, m in enumerate(members):
                bank.write(W[k:k + 1], [A[k]], keys, first=m)
            bank.sync()

        def ranges():
            for k, first, n in runs:
                bank.read_prepare_write(A[k:k + n], keys, first=first, download=False)
            for k, first, n in runs:
                bank.write(W[k:k + n], A[k:k + n], keys, first=first)
            bank.sync()

        def the_list():
            bank.read_prepare_write_list(members, A, keys, download=False)
            bank.write_list(members, W, A, keys)
            bank.sync()

        legs = {"singles": singles, "ranges": ranges, "list": the_list}
        for m in range(M):   # both banks from the same rows: the timed steps before have changed the bank's
            twin.load_encrypted(m, bank.store_encrypted(m))
        want = np.stack([twin.read_prepare_write([A[k]], keys, first=m)[0] for k, m in enumerate(members)])
        equal = bool(np.array_equal(bank.read_prepare_write_list(members, A, keys), want))
        for k, m in enumerate(members):
            twin.write(W[k:k + 1], [A[k]], keys, first=m)
        bank.write_list(members, W, A, keys)
        # (rows of every member; the tree of the named ones: a member that is not named keeps the tree of its own last write, which the
        # two banks did at different times)
        equal = equal and all(np.array_equal(bank.store_encrypted(m), twin.store_encrypted(m)) for m in range(M))
        equal = equal and (args.log_max_addr <= 12 or all(np.array_equal(bank.tree(m), twin.tree(m)) for m in members))
        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        t = {k: [] for k in legs}
        for _ in range(args.reps):            # alternating: one repetition of every leg in turn
            for name, fn in legs.items():
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn()
                t[name].append((time.perf_counter() - t0) / args.iters)
        s = {k: summarise(v) for k, v in t.items()}
        best = min(("singles", "ranges"), key=lambda k: s[k]["median_ms"])
        spread = s[best]["spread_rel"]
        gain = s[best]["median_ms"] / s["list"]["median_ms"]
        # the launch profile of one step of the lists: where its device time goes
        bank.profile_enable(True)
        bank.profile_reset()
        the_list()
        prof = {c: bank.profile_get(c) for c in CLASSES}
        bank.profile_enable(False)
        # ("keyswitch" and "ext_product" include their single-launch forms; the rows' chain is a class of its own)
        total = sum(prof[c]["ms"] for c in ("prepare", "read_chain_launch", "write_chain_launch", "ext_product", "keyswitch", "elementwise"))
        entry = {"members": members, "ranges_leg_calls": [[first, n] for _, first, n in runs], "list_equal_to_single_operations": equal,
                 "legs": s, "better_baseline": best, "baseline_spread_rel": spread, "list_speedup_over_better_baseline": gain,
                 "list_speedup_over_singles": s["singles"]["median_ms"] / s["list"]["median_ms"],
                 "list_speedup_over_ranges": s["ranges"]["median_ms"] / s["list"]["median_ms"],
                 "accept_exceeds_better_baseline_by_more_than_spread": bool(gain > 1.0 + spread),
                 "profile_of_one_list": prof, "profile_device_ms": total,
                 "row_chains_share_of_device_time": (prof["read_chain_launch"]["ms"] + prof["write_chain_launch"]["ms"]) / total if total > 0 else None}
        result["lists"][spec] = entry
        print(f"2^{args.log_max_addr} M={M} list [{spec}]: singles {s['singles']['median_ms']:.3f} ms  ranges {s['ranges']['median_ms']:.3f} ms  "
              f"list {s['list']['median_ms']:.3f} ms  gain over {best} {gain:.3f}  spread {spread:.3f}  equal {equal}  "
              f"row chains {prof['read_chain_launch']['ms'] + prof['write_chain_launch']['ms']:.3f} of {total:.3f} ms", flush=True)
    result["stats"] = {"tail": bank.tail_stats(), "mid": bank.mid_stats(), "roundoff_max": bank.roundoff_max(check=False)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
