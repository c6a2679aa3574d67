#!/usr/bin/env python3
"""Throughput of M RAMs under one key set: fheram_bank against what a host could do before it.

Legs (per member count M, one GPU):
  seq      M standalone contexts driven one after the other, every operation followed by fheram_sync   (baseline a)
  threads  the same M contexts driven from M host threads at once, each op followed by fheram_sync      (baseline b)
  bank     one fheram_bank, every operation on the full range, followed by fheram_bank_sync             (candidate)
Units: the step read + read_prepare_write + write per member, and read alone.

The baseline legs use only the API that existed before the bank, and run in a worker process that loads the library named by
--baseline-lib (a build of the parent commit); the candidate leg runs in a second worker on this tree's library.  Both workers stay
alive for the whole run and the driver alternates between them, repetition by repetition, so baseline and candidate see the same
machine state.  Inputs are synthetic normalised limbs from fixed seeds (as bench.py's), identical in both workers; after the first step
the candidate's results and rows are compared once with the baseline's by SHA-256.

Reported per M and unit: the median of --reps repetitions of every leg (host clock around work that ends in a sync), the spread of
the repeated baseline legs (p10..p90 of the repetitions, relative to the median), the fallbacks the threaded leg's contexts took
(fheram_tail_stats / fheram_mid_stats), and the verdicts of the acceptance rule: at M = 1 the bank within the spread of a plain context,
at M >= 2 the bank's step throughput above the better baseline by more than the spread.

  python tools/bank_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 18 --members 1,2,4,8 --out profiles/bank_2p18.json
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 4096


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int64).tobytes()).hexdigest()


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


# ---- worker -------------------------------------------------------------------------------------------------------------------------
class Worker:
    def __init__(self):
        from _pkg import load_package
        self.pkg = load_package()
        self.pkg.library()
        self.has_bank = hasattr(self.pkg, "RamBank") and hasattr(self.pkg.library(), "fheram_bank_create")
        self.rams, self.bank = [], None

    def setup(self, log_max_addr, M, ws, want):
        pkg = self.pkg
        self.teardown()
        self.M, self.ws = M, ws
        p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        self.p = p
        rng = np.random.default_rng(1234)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N),
                                               synth(rng, 4 * 5 * 2 * N))
        n_digits = p.base2d().as_1d().size()
        rng = np.random.default_rng(4321)
        self.addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(M)]
        self.words = synth(rng, (M, ws, p.glwe_len()))
        rows = [synth(rng, (ws, p.rows(), p.glwe_len())) for _ in range(M)]
        out = {"has_bank": self.has_bank, "lib": os.path.relpath(pkg.library_path(), ROOT)}
        if want == "contexts":
            self.rams = [pkg.Ram(p, 0) for _ in range(M)]
            for m, r in enumerate(self.rams):
                r.load_encrypted(rows[m])
                r._use_keys(self.keys)
            out["device"] = self.rams[0].device_info()
        else:
            self.bank = pkg.RamBank(p, M)
            for m in range(M):
                self.bank.load_encrypted(m, rows[m])
            self.bank._use_keys(self.keys)
        return out

    def teardown(self):
        self.rams, self.bank = [], None

    # one unit on context m / on the bank, every op followed by a sync
    def _ctx_unit(self, m, unit):
        r, a, k = self.rams[m], self.addrs[m], self.keys
        r.read(a, k, download=False)
        r.sync()
        if unit == "step":
            r.read_prepare_write(a, k, download=False)
            r.sync()
            r.write(self.words[m], a, k)
            r.sync()

    def _bank_unit(self, unit):
        b, k = self.bank, self.keys
        b.read(self.addrs, k, download=False)
        b.sync()
        if unit == "step":
            b.read_prepare_write(self.addrs, k, download=False)
            b.sync()
            b.write(self.words, self.addrs, k)
            b.sync()

    def leg(self, kind, unit, iters):
        if kind == "seq":
            t0 = time.perf_counter()
            for _ in range(iters):
                for m in range(self.M):
                    self._ctx_unit(m, unit)
            return time.perf_counter() - t0
        if kind == "bank":
            t0 = time.perf_counter()
            for _ in range(iters):
                self._bank_unit(unit)
            return time.perf_counter() - t0
        start = threading.Barrier(self.M + 1)

        def drive(m):
            start.wait()
            for _ in range(iters):
                self._ctx_unit(m, unit)

        ths = [threading.Thread(target=drive, args=(m,)) for m in range(self.M)]
        for t in ths:
            t.start()
        start.wait()
        t0 = time.perf_counter()
        for t in ths:
            t.join()
        return time.perf_counter() - t0

    def first_step_digests(self):
        """read, read_prepare_write, write on the fresh state: what the other worker must reproduce"""
        d = []
        if self.bank is not None:
            rd = self.bank.read(self.addrs, self.keys)
            pw = self.bank.read_prepare_write(self.addrs, self.keys)
            self.bank.write(self.words, self.addrs, self.keys)
            for m in range(self.M):
                d.append([sha(rd[m]), sha(pw[m]), sha(self.bank.store_encrypted(m))])
        else:
            for m, r in enumerate(self.rams):
                rd = sha(r.read(self.addrs[m], self.keys))
                pw = sha(r.read_prepare_write(self.addrs[m], self.keys))
                r.write(self.words[m], self.addrs[m], self.keys)
                d.append([rd, pw, sha(r.store_encrypted())])
        return d

    def stats(self):
        if self.bank is not None:
            return {"tail": self.bank.tail_stats(), "mid": self.bank.mid_stats(), "roundoff_max": self.bank.roundoff_max(check=False)}
        t = [r.tail_stats() for r in self.rams]
        m = [r.mid_stats() for r in self.rams]
        return {"tail": {k: sum(x[k] for x in t) for k in ("launches", "fallbacks")},
                "mid": {k: sum(x[k] for x in m) for k in ("launches", "fallbacks")},
                "roundoff_max": max(r.roundoff_max(check=False) for r in self.rams)}


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
            res = getattr(w, op)(**cmd)
            out.write(json.dumps({"ok": True, "res": res}) + "\n")
        except Exception as e:   # reported to the driver, which stops
            out.write(json.dumps({"ok": False, "err": f"{type(e).__name__}: {e}"}) + "\n")
        out.flush()
    w.teardown()


# ---- driver -------------------------------------------------------------------------------------------------------------------------
class Remote:
    def __init__(self, lib):
        env = dict(os.environ)
        if lib:
            env["FHERAM_LIB"] = os.path.abspath(lib)
        else:
            env.pop("FHERAM_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, env=env, cwd=ROOT)

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
    ap.add_argument("--baseline-lib", default=None, help="libfheram.so built from the parent commit (default: this tree's library, which "
                                                         "makes the baseline legs a self-comparison, recorded as such)")
    ap.add_argument("--candidate-lib", default=None, help="library of the bank leg (default: this tree's); a parent build here measures the bank "
                                                          "leg of that build, for comparing two builds' banks in one session")
    ap.add_argument("--log-max-addr", type=int, default=18)
    ap.add_argument("--members", default="1,2,4,8")
    ap.add_argument("--word-size", type=int, default=4)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--iters", type=int, default=4, help="units per timed repetition")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker_main()
    base, cand = Remote(args.baseline_lib), Remote(args.candidate_lib)
    result = {"tool": "tools/bank_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "reps": args.reps,
              "iters_per_rep": args.iters, "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around synced ops",
              "spread": "p10..p90 of the repetitions of a leg over its median", "members": {}}
    try:
        for M in [int(x) for x in args.members.split(",")]:
            sb = base.call("setup", log_max_addr=args.log_max_addr, M=M, ws=args.word_size, want="contexts")
            sc = cand.call("setup", log_max_addr=args.log_max_addr, M=M, ws=args.word_size, want="bank")
            result["device"] = sb.get("device")
            result["baseline_lib"], result["candidate_lib"] = sb["lib"], sc["lib"]
            result["baseline_lib_has_bank"] = sb["has_bank"]
            same = base.call("first_step_digests") == cand.call("first_step_digests")
            entry = {"first_step_equal_to_baseline": same, "units": {}}
            for unit in ("step", "read"):
                legs = [(base, "seq"), (base, "threads"), (cand, "bank")]
                for r, kind in legs:
                    r.call("leg", kind=kind, unit=unit, iters=args.warmup)
                t = {"seq": [], "threads": [], "bank": []}
                for _ in range(args.reps):            # alternating: one repetition of every leg in turn
                    for r, kind in legs:
                        t[kind].append(r.call("leg", kind=kind, unit=unit, iters=args.iters) / args.iters)
                s = {k: summarise(v) for k, v in t.items()}
                best = min(("seq", "threads"), key=lambda k: s[k]["median_ms"])
                spread = max(s["seq"]["spread_rel"], s["threads"]["spread_rel"])
                gain = s[best]["median_ms"] / s["bank"]["median_ms"]
                u = {"per_unit_of_M_members": s, "better_baseline": best, "baseline_spread_rel": spread, "bank_speedup_over_better_baseline": gain,
                     "bank_speedup_over_seq": s["seq"]["median_ms"] / s["bank"]["median_ms"],
                     "units_per_s_bank": M / (s["bank"]["median_ms"] * 1e-3), "units_per_s_better_baseline": M / (s[best]["median_ms"] * 1e-3)}
                if M == 1:
                    u["accept_within_spread_of_plain_context"] = abs(s["bank"]["median_ms"] / s["seq"]["median_ms"] - 1.0) <= s["seq"]["spread_rel"]
                else:
                    u["accept_exceeds_better_baseline_by_more_than_spread"] = gain > 1.0 + spread
                entry["units"][unit] = u
                print(f"2^{args.log_max_addr} M={M} {unit}: seq {s['seq']['median_ms']:.3f} ms  threads {s['threads']['median_ms']:.3f} ms  "
                      f"bank {s['bank']['median_ms']:.3f} ms  gain over {best} {gain:.3f}  spread {spread:.3f}", flush=True)
            entry["baseline_contexts_stats"] = base.call("stats")
            entry["bank_stats"] = cand.call("stats")
            result["members"][str(M)] = entry
            base.call("teardown")
            cand.call("teardown")
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
