#!/usr/bin/env python3
"""The derivations of a VM step as ONE launch (fheram_bank_derive_list) against the fewest calls of the entry points before it, on a bank of
three (register file, ROM, data memory), word size 4, synthetic normalised limbs.

Step legs (the byte store SB of tools/lanes_bench.py's device leg; the register word is a read-list entry of member 0, the store goes to member 2):
  calls  (a) a worker process of its own on the library named by --baseline-lib (a build of the parent commit): derive_addresses(first_bits =
             [2, 0]) — two launches — and derive_selector_fields — two launches —, then read_list, read_prepare_write_list, select_lanes over
             store_merge_lanes (all out = NULL), write_list_selected, one sync
  list   (b) this tree's library in a second worker: the same step with ONE derive_list for the two addresses and the [2, 2] field selector

Derivations alone, each followed by a sync, same two workers:
  sb     the SB step's set: two addresses (first bits 2 and 0) and the [2, 2] field selector — 4 launches against 1
  full   a full step's set: six addresses at three distinct first bits, one [2, 2] field selector and one plain 5-bit selector — derive_addresses
         (3 launches), derive_selector_fields (2), derive_selectors (1) against 1

Method as tools/lanes_bench.py: host clock around calls that end in a sync, the legs alternated repetition by repetition, the median of --reps
repetitions, the p10..p90 spread of the baseline.  Inputs are synthetic normalised limbs from fixed seeds, identical in both workers.

Acceptance: list beats calls by more than calls' spread.

  python tools/derive_list_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/derive_list_2p14.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 4096
REGS, DATA = 0, 2
FULL_FIRST = [2, 2, 0, 0, 1, 1]   # the first bits of the full set's six addresses


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


class Worker:
    def setup(self, log_max_addr, ws):
        from _pkg import load_package
        pkg = self.pkg = load_package()
        p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        rng = np.random.default_rng(1234)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
        bank = self.bank = pkg.RamBank(p, 3, 0)
        for m in range(3):
            bank.load_encrypted(m, synth(rng, (ws, p.rows(), p.glwe_len())))
        bank._use_keys(self.keys)
        fu_len = pkg.library().fheram_fheuint_ggsw_len(None)
        n_bits = log_max_addr + 2
        self.fus = [pkg.FheUintPrepared.from_host(bank, synth(rng, (n_bits, fu_len))) for _ in range(3)]   # byte address, register address, op
        self.addrs = [pkg.Address.alloc(bank) for _ in range(6)]
        self.sel, self.sel5 = bank.selector_fields([2, 2]), bank.selector(5)
        self.has_list = hasattr(pkg.library(), "fheram_bank_derive_list")
        bank.sync()
        return {"lib": pkg.library_path(), "has_derive_list": self.has_list, "address_digits": p.base2d().as_1d().size()}

    def derive(self, kind, which):
        """the derivations of set `which` ("sb" / "full"), by the existing calls or by one derive list; nothing waits"""
        pkg, bank, fus, a = self.pkg, self.bank, self.fus, self.addrs
        if kind == "calls":
            if which == "sb":
                bank.derive_addresses(fus[:2], a[:2], first_bits=[2, 0])
            else:
                bank.derive_addresses([fus[i % 2] for i in range(6)], a, first_bits=FULL_FIRST)
                bank.derive_selectors([fus[2]], [0], [self.sel5])
            bank.derive_selector_fields(self.sel, [fus[2], fus[0]], [0, 0])
        else:
            D = pkg.Derive
            if which == "sb":
                items = [D.address(fus[0], a[0], 2), D.address(fus[1], a[1], 0)]
            else:
                items = [D.address(fus[i % 2], a[i], FULL_FIRST[i]) for i in range(6)] + [D.selector(fus[2], self.sel5, 0)]
            bank.derive_list(items + [D.fields(self.sel, [fus[2], fus[0]], [0, 0])])

    def leg(self, kind, what):
        pkg, bank, keys, S = self.pkg, self.bank, self.keys, self.pkg.Src
        t0 = time.perf_counter()
        if what == "step":
            self.derive(kind, "sb")
            bank.read_list([REGS], [self.addrs[1]], keys, download=False)
            bank.read_prepare_write_list([DATA], [self.addrs[0]], keys, download=False)
            bank.select_lanes([self.sel], [pkg.store_merge_lanes(S.list(0), S.member(DATA))], download=False)
            bank.write_list_selected([DATA], [0], [self.addrs[0]], keys)
        else:
            self.derive(kind, what)
        bank.sync()
        return time.perf_counter() - t0

    def profile(self, kind, what):
        self.bank.profile_enable(True)
        self.bank.profile_reset()
        self.leg(kind, what)
        out = {c: self.bank.profile_get(c) for c in ("derive", "select_pack", "prepare", "ext_product", "keyswitch", "elementwise")}
        self.bank.profile_enable(False)
        out["roundoff_max"] = self.bank.roundoff_max(check=False)
        return out


def worker_main():
    out = os.fdopen(os.dup(1), "w")   # replies on the original stdout; anything a library prints goes to stderr
    os.dup2(2, 1)
    w = Worker()
    for line in sys.stdin:
        cmd = json.loads(line)
        try:
            op = cmd.pop("op")
            if op == "quit":
                break
            out.write(json.dumps({"ok": True, "res": getattr(w, op)(**cmd)}) + "\n")
        except Exception as e:   # reported to the driver, which stops
            out.write(json.dumps({"ok": False, "err": f"{type(e).__name__}: {e}"}) + "\n")
        out.flush()


class Remote:
    def __init__(self, lib):
        env = dict(os.environ)
        if lib:
            env["FHERAM_LIB"] = os.path.abspath(lib)
        else:
            env.pop("FHERAM_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)

    def call(self, op, **kw):
        self.p.stdin.write(json.dumps(dict(op=op, **kw)) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"worker died during {op} (exit status {self.p.poll()})")
        r = json.loads(line)
        if not r["ok"]:
            raise RuntimeError(f"worker failed in {op}: {r['err']}")
        return r["res"]

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"op": "quit"}) + "\n")
            self.p.stdin.flush()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def pct(xs, q):
    return float(np.percentile(np.asarray(xs), q))


def summarise(xs):
    med = float(np.median(xs))
    return {"median_ms": med * 1e3, "min_ms": min(xs) * 1e3, "max_ms": max(xs) * 1e3, "p10_ms": pct(xs, 10) * 1e3, "p90_ms": pct(xs, 90) * 1e3,
            "spread_rel": (pct(xs, 90) - pct(xs, 10)) / med}


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
        return worker_main()
    base, cand = Remote(args.baseline_lib), Remote(None)
    result = {"tool": "tools/derive_list_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "reps": args.reps,
              "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in a sync",
              "spread": "p10..p90 of the repetitions of a leg over its median"}
    try:
        sb = base.call("setup", log_max_addr=args.log_max_addr, ws=args.word_size)
        sc = cand.call("setup", log_max_addr=args.log_max_addr, ws=args.word_size)
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(sb["lib"], ROOT),
                      candidate_lib=os.path.relpath(sc["lib"], ROOT), baseline_lib_has_derive_list=sb["has_derive_list"], address_digits=sc["address_digits"])
        legs = [(base, "calls"), (cand, "list")]
        for what in ("step", "sb", "full"):
            for _ in range(args.warmup):
                for r, kind in legs:
                    r.call("leg", kind=kind, what=what)
            t = {"calls": [], "list": []}
            for _ in range(args.reps):   # alternating: one repetition of each leg in turn
                for r, kind in legs:
                    t[kind].append(r.call("leg", kind=kind, what=what))
            s = {k: summarise(v) for k, v in t.items()}
            gain = s["calls"]["median_ms"] / s["list"]["median_ms"]
            result[what] = {"legs": s, "baseline_spread_rel": s["calls"]["spread_rel"], "list_speedup_over_calls": gain,
                            "saved_ms": s["calls"]["median_ms"] - s["list"]["median_ms"],
                            "accept_beats_calls_by_more_than_spread": bool(gain > 1.0 + s["calls"]["spread_rel"]),
                            "launch_profile": {kind: r.call("profile", kind=kind, what=what) for r, kind in legs}}
            print(f"2^{args.log_max_addr} {what}: calls {s['calls']['median_ms']:.3f} ms  list {s['list']['median_ms']:.3f} ms  gain {gain:.2f}  "
                  f"calls spread {s['calls']['spread_rel']:.3f}", flush=True)
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
