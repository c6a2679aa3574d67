#!/usr/bin/env python3
"""The reads of a VM step as ONE operation (fheram_bank_read_mix) against the parent's forms, word size 4, synthetic normalised limbs.

Workers (a process each):
  seq     the library named by --baseline-lib (a build of the parent commit): a bank of ONE plus a 12-bit table and a 5-bit register file,
          the reads as single calls one behind the other
  member  the same library: a bank of TWO whose member 0 is the ROM (DESIGN.md 18's second form of a fetch)
  mix     this tree's library: the bank of `seq`, the reads as one read_mix

Legs:
  fetch_data  a fetch plus a data read, Y = 8 ciphertexts (the tail form): mix {list [0], table} against BOTH parent forms — seq: table_read
              then read_list [0]; member: read_list [0, 1]
  step        a full step's reads, Y = 16 (the unfused form): mix {list [0], table, regs x 2} against seq: table_read, regs_read of two
              selectors, read_list [0]

Method as tools/table_bench.py: host clock around calls that end in ONE sync (every call before it has out = NULL), the legs alternated
repetition by repetition, the median of --reps repetitions with p10..p90.  Inputs are synthetic normalised limbs from fixed seeds.

Acceptance: the mix counts as faster than a parent leg only if it beats that leg's median by more than that leg's own
p10..p90 spread.

  python tools/mix_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/mix_2p14.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from table_bench import Remote, summarise, synth  # noqa: E402

N = 4096
TABLE_BITS, REGS_BITS = 12, 5
PROFILE_CLASSES = ("prepare", "ext_product", "keyswitch", "keyswitch_tail_launch", "keyswitch_mid_launch", "elementwise", "read_chain_launch")


class Worker:
    def setup(self, kind, log_max_addr, ws):
        from _pkg import load_package
        pkg = self.pkg = load_package()
        self.kind = kind
        p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        rng = np.random.default_rng(4321)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
        members = 2 if kind == "member" else 1
        bank = self.bank = pkg.RamBank(p, members, 0)
        for m in range(members):
            bank.load_encrypted(m, synth(rng, (ws, p.rows(), p.glwe_len())))
        bank._use_keys(self.keys)
        n_digits = p.base2d().as_1d().size()
        self.addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(2)]
        digits = {}
        if kind != "member":
            self.table = bank.table(TABLE_BITS)
            self.table.load(synth(rng, (ws, p.glwe_len())))
            self.rf = bank.regfile(REGS_BITS)
            self.rf.load(synth(rng, (ws, p.glwe_len())))
            digits = {"table": bank.table_selector(TABLE_BITS).n_digits(), "regs": bank.selector(REGS_BITS).n_digits()}
            self.fetch = bank.table_selector(TABLE_BITS, list(synth(rng, (digits["table"], p.ggsw_len()))))
            self.rs = [pkg.Selector.from_digits(bank, REGS_BITS, list(synth(rng, (digits["regs"], p.ggsw_len())))) for _ in range(2)]
        for what in self.legs():   # once through, so that every buffer a leg grows on first use exists
            self.leg(what)
        return {"lib": pkg.library_path(), "has_mix": hasattr(pkg.library(), "fheram_bank_read_mix"), "members": members, "address_digits": n_digits,
                "selector_digits": digits}

    def legs(self):
        return ["fetch_data"] if self.kind == "member" else ["fetch_data", "step"]

    def leg(self, what):
        bank, keys, a = self.bank, self.keys, self.addrs
        t0 = time.perf_counter()
        if self.kind == "member":
            bank.read_list([0, 1], [a[0], a[1]], keys, download=False)
        elif self.kind == "seq":
            bank.table_read([self.table], [self.fetch], download=False)
            if what == "step":
                self.rf.read(self.rs, download=False)
            bank.read_list([0], [a[1]], keys, download=False)
        else:
            bank.read_mix(list=([0], [a[1]]), tables=([self.table], [self.fetch]), regs=(self.rf, self.rs) if what == "step" else None, download=False)
        bank.sync()
        return time.perf_counter() - t0

    def profile(self, what):
        self.bank.profile_enable(True)
        self.bank.profile_reset()
        self.leg(what)
        out = {c: self.bank.profile_get(c) for c in PROFILE_CLASSES}
        self.bank.profile_enable(False)
        out["roundoff_max"] = self.bank.roundoff_max(check=False)
        out["tail_stats"] = self.bank.tail_stats()
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


class MixRemote(Remote):
    """tools/table_bench.py's worker handle, started on this file"""

    def __init__(self, lib):
        import subprocess
        env = dict(os.environ)
        if lib:
            env["FHERAM_LIB"] = os.path.abspath(lib)
        else:
            env.pop("FHERAM_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)


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
    workers = {"seq": MixRemote(args.baseline_lib), "member": MixRemote(args.baseline_lib), "mix": MixRemote(None)}
    result = {"tool": "tools/mix_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "table_bits": TABLE_BITS, "regs_bits": REGS_BITS,
              "reps": args.reps, "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in one sync",
              "spread": "p10..p90 of the repetitions of a leg over its median",
              "rule": "the mix counts as faster than a parent leg only if it beats that leg's median by more than that leg's own spread"}
    try:
        info = {k: r.call("setup", kind=k, log_max_addr=args.log_max_addr, ws=args.word_size) for k, r in workers.items()}
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(info["seq"]["lib"], ROOT),
                      candidate_lib=os.path.relpath(info["mix"]["lib"], ROOT), baseline_lib_has_mix=info["seq"]["has_mix"],
                      selector_digits=info["mix"]["selector_digits"], address_digits=info["mix"]["address_digits"], members={k: v["members"] for k, v in info.items()})
        for what, kinds in (("fetch_data", ("seq", "member", "mix")), ("step", ("seq", "mix"))):
            for _ in range(args.warmup):
                for k in kinds:
                    workers[k].call("leg", what=what)
            t = {k: [] for k in kinds}
            for _ in range(args.reps):   # alternating: one repetition of each leg in turn
                for k in kinds:
                    t[k].append(workers[k].call("leg", what=what))
            s = {k: summarise(v) for k, v in t.items()}
            rows = {}
            for k in kinds:
                if k == "mix":
                    continue
                gain = s[k]["median_ms"] / s["mix"]["median_ms"]
                rows[k] = {"mix_speedup": gain, "saved_ms": s[k]["median_ms"] - s["mix"]["median_ms"], "parent_spread_rel": s[k]["spread_rel"],
                           "accept_beats_parent_by_more_than_its_spread": bool(gain > 1.0 + s[k]["spread_rel"])}
                print(f"2^{args.log_max_addr} {what}: {k} {s[k]['median_ms']:.3f} ms  mix {s['mix']['median_ms']:.3f} ms  gain {gain:.3f}  "
                      f"{k} spread {s[k]['spread_rel']:.3f}  {'met' if rows[k]['accept_beats_parent_by_more_than_its_spread'] else 'NOT met'}", flush=True)
            result[what] = {"ciphertexts": (2 if what == "fetch_data" else 4) * args.word_size, "legs": s, "against": rows,
                            "launch_profile": {k: workers[k].call("profile", what=what) for k in kinds}}
    finally:
        for r in workers.values():
            r.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
