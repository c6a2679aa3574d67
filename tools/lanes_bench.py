#!/usr/bin/env python3
"""The byte store (SB) of a VM step on a bank of three — register file, ROM, data memory — with the store merge on the device
(fheram_bank_select_lanes, a [2, 2] field selector, fheram_address_derive_at) against the only route the entry points before them offer.

Legs (one GPU, both on a bank of three members; the register word is a read-list entry of member 0, the store goes to member 2):
  host    (a) only entry points the parent commit has, in a worker process of its own on the library named by --baseline-lib (a build of the
              parent): derive_addresses; derive_selectors (four contiguous bits of ONE integer: the parent cannot take op and offset from
              two); read_list with download; read_prepare_write_list with download; the 14 store-merge candidates shuffled in numpy; select with
              HOST candidates (out = NULL); write_list_selected; sync
  device  (b) this tree's library in a second worker: derive_addresses(first_bits = [2]); derive_selector_fields; read_list(out = NULL);
              read_prepare_write_list(out = NULL); select_lanes over store_merge_lanes (out = NULL); write_list_selected; one sync

Method as tools/select_bench.py and tools/bank_bench.py: host clock around calls that end in a sync, the legs alternated repetition by
repetition, the median of --reps repetitions, the p10..p90 spread of the baseline.  Inputs are synthetic normalised limbs from fixed seeds,
identical in both workers.

Acceptance: device beats host by more than host's spread.

  python tools/lanes_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/store_merge_2p14.json
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


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


def host_candidates(x, y):
    """the 14 store-merge candidates [14][ws][GLWE] from the downloaded words x (register) and y (memory): whole byte ciphertexts moved"""
    zero = np.zeros_like(y)
    out = []
    for offset in range(4):
        sb = y.copy()
        sb[offset] = x[0]
        sh = zero
        if offset in (0, 2):
            sh = y.copy()
            sh[offset], sh[offset + 1] = x[0], x[1]
        out += [y, sb, sh, x if offset == 0 else zero]
    return np.stack(out[:14])


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
        self.addrs = [pkg.Address.alloc(bank) for _ in range(2)]
        self.has_lanes = hasattr(pkg.library(), "fheram_bank_select_lanes")
        self.sel = bank.selector_fields([2, 2]) if self.has_lanes else None
        self.sel4 = bank.selector(4)
        bank.sync()
        return {"lib": pkg.library_path(), "has_lanes": self.has_lanes}

    def leg(self, kind):
        pkg, bank, keys, S = self.pkg, self.bank, self.keys, self.pkg.Src
        t0 = time.perf_counter()
        if kind == "host":
            bank.derive_addresses(self.fus[:2], self.addrs)
            bank.derive_selectors([self.fus[2]], [0], [self.sel4])
            x = bank.read_list([REGS], [self.addrs[1]], keys)[0]
            y = bank.read_prepare_write_list([DATA], [self.addrs[0]], keys)[0]
            cands = host_candidates(x, y)
            bank.select([self.sel4], [[S.host(j) for j in range(14)]], host_words=cands, download=False)
        else:
            bank.derive_addresses(self.fus[:2], self.addrs, first_bits=[2, 0])
            bank.derive_selector_fields(self.sel, [self.fus[2], self.fus[0]], [0, 0])
            bank.read_list([REGS], [self.addrs[1]], keys, download=False)
            bank.read_prepare_write_list([DATA], [self.addrs[0]], keys, download=False)
            bank.select_lanes([self.sel], [pkg.store_merge_lanes(S.list(0), S.member(DATA))], download=False)
        bank.write_list_selected([DATA], [0], [self.addrs[0]], keys)
        bank.sync()
        return time.perf_counter() - t0

    def profile(self, kind):
        self.bank.profile_enable(True)
        self.bank.profile_reset()
        self.leg(kind)
        out = {c: self.bank.profile_get(c) for c in ("select_pack", "derive", "prepare", "ext_product", "keyswitch", "elementwise")}
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
    result = {"tool": "tools/lanes_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "reps": args.reps, "step": "SB store: register word of member 0 into member 2",
              "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in a sync",
              "spread": "p10..p90 of the repetitions of a leg over its median"}
    try:
        sb = base.call("setup", log_max_addr=args.log_max_addr, ws=args.word_size)
        sc = cand.call("setup", log_max_addr=args.log_max_addr, ws=args.word_size)
        result["baseline_lib"], result["candidate_lib"], result["baseline_lib_has_lanes"] = sb["lib"], sc["lib"], sb["has_lanes"]
        legs = [(base, "host"), (cand, "device")]
        for _ in range(args.warmup):
            for r, kind in legs:
                r.call("leg", kind=kind)
        t = {"host": [], "device": []}
        for _ in range(args.reps):   # alternating: one repetition of each leg in turn
            for r, kind in legs:
                t[kind].append(r.call("leg", kind=kind))
        s = {k: summarise(v) for k, v in t.items()}
        gain = s["host"]["median_ms"] / s["device"]["median_ms"]
        result["store_merge_step"] = {"legs": s, "baseline_spread_rel": s["host"]["spread_rel"], "device_speedup_over_host": gain,
                                      "accept_beats_host_by_more_than_spread": bool(gain > 1.0 + s["host"]["spread_rel"]),
                                      "launch_profile": {kind: r.call("profile", kind=kind) for r, kind in legs}}
        print(f"2^{args.log_max_addr} SB store: host {s['host']['median_ms']:.3f} ms  device {s['device']['median_ms']:.3f} ms  gain {gain:.2f}  "
              f"host spread {s['host']['spread_rel']:.3f}", flush=True)
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
