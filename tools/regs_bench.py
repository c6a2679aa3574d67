#!/usr/bin/env python3
"""The register traffic of a VM step on a bank's register file (fheram_bank_regs_*) against the register file held as a bank member, word
size 4, synthetic normalised limbs.

Step legs (a step reads rs1 and rs2, fetches from the ROM and the data memory, and writes rd):
  member (a) a worker process of its own on the library named by --baseline-lib (a build of the parent commit): a bank of THREE whose member 0
             is the register file: read_list [0, 0, 1, 2], read_prepare_write_list [0], write_list [0] of a host word, one sync
  regs   (b) this tree's library in a second worker: a bank of TWO plus a 5-bit register file: regs_read of two selectors, read_list [0, 1],
             regs_read_prepare_write, regs_write(HOST), one sync

Register traffic alone ("traffic"), same two workers: (a) read_list [0, 0], read_prepare_write_list [0], write_list [0]; (b) regs_read of two
selectors, regs_read_prepare_write, regs_write(HOST); each followed by one sync.

Method as tools/derive_list_bench.py: host clock around calls that end in a sync (every call before it has out = NULL), the legs alternated
repetition by repetition, the median of --reps repetitions, the p10..p90 spread of the baseline.  Inputs are synthetic normalised limbs from
fixed seeds.

Acceptance: regs beats member by more than member's spread.

  python tools/regs_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/regs_2p14.json
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
BITS = 5


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


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
        self.addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(4)]
        self.word = synth(rng, (1, ws, p.glwe_len()))
        if kind == "regs":
            self.rf = bank.regfile(BITS)
            self.rf.load(synth(rng, (ws, p.glwe_len())))
            self.sels = [pkg.Selector.from_digits(bank, BITS, list(synth(rng, (2, p.ggsw_len())))) for _ in range(3)]
        # once through, so that every buffer either leg grows on first use exists
        self.leg("step")
        return {"lib": pkg.library_path(), "has_regs": hasattr(pkg.library(), "fheram_bank_regs_create"), "members": members, "address_digits": n_digits}

    def leg(self, what):
        bank, keys, a = self.bank, self.keys, self.addrs
        t0 = time.perf_counter()
        if self.kind == "member":
            if what == "step":
                bank.read_list([0, 0, 1, 2], [a[0], a[1], a[2], a[3]], keys, download=False)
            else:
                bank.read_list([0, 0], [a[0], a[1]], keys, download=False)
            bank.read_prepare_write_list([0], [a[0]], keys, download=False)
            bank.write_list([0], self.word, [a[0]], keys)
        else:
            rf, S = self.rf, self.pkg.Src
            rf.read(self.sels[:2], download=False)
            if what == "step":
                bank.read_list([0, 1], [a[2], a[3]], keys, download=False)
            rf.read_prepare_write(self.sels[2], download=False)
            rf.write(self.sels[2], S.host(0), host_words=self.word)
        bank.sync()
        return time.perf_counter() - t0

    def profile(self, what):
        self.bank.profile_enable(True)
        self.bank.profile_reset()
        self.leg(what)
        out = {c: self.bank.profile_get(c) for c in ("prepare", "ext_product", "keyswitch", "elementwise", "read_chain_launch", "write_chain_launch")}
        self.bank.profile_enable(False)
        out["roundoff_max"] = self.bank.roundoff_max(check=False)
        return out


def worker_main(w=None):
    """w: the worker object whose methods the driver calls (tools/scratch_bench.py brings its own)"""
    out = os.fdopen(os.dup(1), "w")   # replies on the original stdout; anything a library prints goes to stderr
    os.dup2(2, 1)
    w = w or Worker()
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
    def __init__(self, lib, script=None):
        """script: the tool whose --worker the process runs (this one unless given)"""
        env = dict(os.environ)
        if lib:
            env["FHERAM_LIB"] = os.path.abspath(lib)
        else:
            env.pop("FHERAM_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(script or __file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)

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
    result = {"tool": "tools/regs_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "regs_bits": BITS, "reps": args.reps,
              "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in a sync",
              "spread": "p10..p90 of the repetitions of a leg over its median"}
    try:
        sb = base.call("setup", kind="member", log_max_addr=args.log_max_addr, ws=args.word_size)
        sc = cand.call("setup", kind="regs", log_max_addr=args.log_max_addr, ws=args.word_size)
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(sb["lib"], ROOT),
                      candidate_lib=os.path.relpath(sc["lib"], ROOT), baseline_lib_has_regs=sb["has_regs"], address_digits=sc["address_digits"],
                      members={"member": sb["members"], "regs": sc["members"]})
        legs = [(base, "member"), (cand, "regs")]
        for what in ("step", "traffic"):
            for _ in range(args.warmup):
                for r, kind in legs:
                    r.call("leg", what=what)
            t = {"member": [], "regs": []}
            for _ in range(args.reps):   # alternating: one repetition of each leg in turn
                for r, kind in legs:
                    t[kind].append(r.call("leg", what=what))
            s = {k: summarise(v) for k, v in t.items()}
            gain = s["member"]["median_ms"] / s["regs"]["median_ms"]
            result[what] = {"legs": s, "baseline_spread_rel": s["member"]["spread_rel"], "regs_speedup_over_member": gain,
                            "saved_ms": s["member"]["median_ms"] - s["regs"]["median_ms"],
                            "accept_beats_member_by_more_than_spread": bool(gain > 1.0 + s["member"]["spread_rel"]),
                            "launch_profile": {kind: r.call("profile", what=what) for r, kind in legs}}
            print(f"2^{args.log_max_addr} {what}: member {s['member']['median_ms']:.3f} ms  regs {s['regs']['median_ms']:.3f} ms  gain {gain:.2f}  "
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
