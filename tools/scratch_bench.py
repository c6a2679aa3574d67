#!/usr/bin/env python3
"""The traffic of a small WRITTEN memory of 4096 words on a wide register file (fheram_bank_regs_create_wide) against the same memory held as
a bank member, word size 4, synthetic normalised limbs.

Legs (one read, one write cycle of a host word, one sync):
  member  (a) a worker process of its own on the library named by --baseline-lib (a build of the parent commit): a bank of THREE whose member 0
              is the small memory: read_list [0], read_prepare_write_list [0], write_list [0] of a host word
  scratch (b) this tree's library in a second worker: a bank of TWO plus a 12-bit wide register file: regs_read of one selector,
              regs_read_prepare_write, regs_write(HOST)

Method as tools/regs_bench.py: host clock around calls that end in a sync (every call before it has out = NULL), the legs alternated
repetition by repetition, the median of --reps repetitions, the p10..p90 spread of the baseline.  Inputs are synthetic normalised limbs from
fixed seeds.  The launch counts of each operation of a leg are recorded beside the times.

Acceptance: scratch beats member by more than member's spread.

  python tools/scratch_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/scratch_2p14.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from regs_bench import N, Remote, summarise, synth, worker_main  # noqa: E402 (the worker protocol and the statistics are regs_bench's)

BITS = 12
CATEGORIES = ("prepare", "ext_product", "keyswitch", "elementwise", "read_chain_launch", "write_chain_launch")


class Worker:
    def setup(self, kind, log_max_addr, ws):
        from _pkg import load_package
        pkg = self.pkg = load_package()
        self.kind = kind
        p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        rng = np.random.default_rng(4321)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
        members = 3 if kind == "member" else 2
        bank = self.bank = pkg.RamBank(p, members, 0)
        for m in range(members):
            bank.load_encrypted(m, synth(rng, (ws, p.rows(), p.glwe_len())))
        bank._use_keys(self.keys)
        n_digits = p.base2d().as_1d().size()
        self.addr = pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len()))))
        self.word = synth(rng, (1, ws, p.glwe_len()))
        sel_digits = 0
        if kind == "scratch":
            self.rf = bank.scratch(BITS)
            self.rf.load(synth(rng, (ws, p.glwe_len())))
            self.sel = bank.table_selector(BITS)
            sel_digits = self.sel.n_digits()
            self.sel = bank.table_selector(BITS, list(synth(rng, (sel_digits, p.ggsw_len()))))
        self.ops = self._member_ops() if kind == "member" else self._scratch_ops()
        self.leg()   # once through, so that every buffer either leg grows on first use exists
        return {"lib": pkg.library_path(), "has_wide": hasattr(pkg.library(), "fheram_bank_regs_create_wide"), "members": members,
                "address_digits": n_digits, "selector_digits": sel_digits}

    def _member_ops(self):
        bank, keys, a = self.bank, self.keys, self.addr
        return [("read", lambda: bank.read_list([0], [a], keys, download=False)),
                ("read_prepare_write", lambda: bank.read_prepare_write_list([0], [a], keys, download=False)),
                ("write", lambda: bank.write_list([0], self.word, [a], keys))]

    def _scratch_ops(self):
        rf, S = self.rf, self.pkg.Src
        return [("read", lambda: rf.read([self.sel], download=False)),
                ("read_prepare_write", lambda: rf.read_prepare_write(self.sel, download=False)),
                ("write", lambda: rf.write(self.sel, S.host(0), host_words=self.word))]

    def leg(self):
        t0 = time.perf_counter()
        for _, op in self.ops:
            op()
        self.bank.sync()
        return time.perf_counter() - t0

    def profile(self):
        """the launches of each operation of the leg, by category, and their sum"""
        bank = self.bank
        bank.profile_enable(True)
        out = {}
        for name, op in self.ops:
            bank.profile_reset()
            op()
            bank.sync()
            cats = {c: bank.profile_get(c) for c in CATEGORIES}
            out[name] = {"launches": sum(v["launches"] for v in cats.values()), "by_category": cats}
        bank.profile_enable(False)
        out["roundoff_max"] = bank.roundoff_max(check=False)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--baseline-lib", default=None, help="libfheram.so built from the parent commit (default: this tree's library, recorded as such)")
    ap.add_argument("--log-max-addr", type=int, default=14)
    ap.add_argument("--word-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker_main(Worker())
    me = os.path.abspath(__file__)
    base, cand = Remote(args.baseline_lib, me), Remote(None, me)
    result = {"tool": "tools/scratch_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "scratch_bits": BITS, "reps": args.reps,
              "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in a sync",
              "spread": "p10..p90 of the repetitions of a leg over its median"}
    try:
        sb = base.call("setup", kind="member", log_max_addr=args.log_max_addr, ws=args.word_size)
        sc = cand.call("setup", kind="scratch", log_max_addr=args.log_max_addr, ws=args.word_size)
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(sb["lib"], ROOT),
                      candidate_lib=os.path.relpath(sc["lib"], ROOT), baseline_lib_has_wide=sb["has_wide"], address_digits=sc["address_digits"],
                      selector_digits=sc["selector_digits"], members={"member": sb["members"], "scratch": sc["members"]})
        legs = [(base, "member"), (cand, "scratch")]
        for _ in range(args.warmup):
            for r, kind in legs:
                r.call("leg")
        t = {"member": [], "scratch": []}
        for _ in range(args.reps):   # alternating: one repetition of each leg in turn
            for r, kind in legs:
                t[kind].append(r.call("leg"))
        s = {k: summarise(v) for k, v in t.items()}
        gain = s["member"]["median_ms"] / s["scratch"]["median_ms"]
        result["traffic"] = {"legs": s, "baseline_spread_rel": s["member"]["spread_rel"], "scratch_speedup_over_member": gain,
                             "saved_ms": s["member"]["median_ms"] - s["scratch"]["median_ms"],
                             "accept_beats_member_by_more_than_spread": bool(gain > 1.0 + s["member"]["spread_rel"]),
                             "launch_profile": {kind: r.call("profile") for r, kind in legs}}
        print(f"2^{args.log_max_addr} traffic: member {s['member']['median_ms']:.3f} ms  scratch {s['scratch']['median_ms']:.3f} ms  gain {gain:.2f}  "
              f"member spread {s['member']['spread_rel']:.3f}", flush=True)
    finally:
        base.close()
        cand.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
