#!/usr/bin/env python3
"""A VM step up to its writes as ONE operation (fheram_bank_read_prepare_write_mix) against the parent's forms, word size 4, synthetic
normalised limbs.  A bank of ONE member (the data memory) plus a 12-bit table (the program) and a 5-bit register file.

Workers (a process each):
  parent  the library named by --baseline-lib (a build of the parent commit)
  mix     this tree's library

Legs (parent form / mix form):
  A  prepare  the write halves' preparation, Y = 8: read_prepare_write_list [data] + regs_read_prepare_write  /  one mix of two prepares
  B  step     a step up to its writes, Y = 24: read_mix(fetch, rs1, rs2, data) + the two preparations  /  one mix of six entries
  C  step5    B without the redundant data read, Y = 20: five entries, the loaded word being the prepared member's old word; measured
              against B's parent leg (no parent form of its own)
  D  whole    B continued through select [MEMBER_RESULT, HOST], write_list_selected and regs_write(REGS_OLD) to one sync: the writes did
              not get slower

Method as tools/mix_bench.py: host clock around calls that end in ONE sync (every call before it has out = NULL), the legs alternated
repetition by repetition, the median of --reps repetitions with p10..p90.  A and B / C end between the two halves, so every repetition is
followed, outside the clock, by the writes that put the member and the register file back into state 0.

Acceptance: the mix counts as faster than the parent leg only if it beats that leg's median by more than that leg's own
p10..p90 spread (A, B); D: not slower than its parent leg by more than that spread.

  python tools/rpw_mix_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/rpw_mix_2p14.json
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
PROFILE_CLASSES = ("prepare", "ext_product", "keyswitch", "keyswitch_tail_launch", "keyswitch_mid_launch", "keyswitch_chain_launch", "elementwise", "read_chain_launch",
                   "write_chain_launch", "select_pack")
LEGS = {"prepare": ("parent", "mix"), "step": ("parent", "mix"), "step5": ("mix",), "whole": ("parent", "mix")}
ENTRIES = {"prepare": 2, "step": 6, "step5": 5, "whole": 6}


class Worker:
    def setup(self, kind, log_max_addr, ws):
        from _pkg import load_package
        pkg = self.pkg = load_package()
        self.kind = kind
        p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        rng = np.random.default_rng(4321)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
        bank = self.bank = pkg.RamBank(p, 1, 0)
        bank.load_encrypted(0, synth(rng, (ws, p.rows(), p.glwe_len())))
        bank._use_keys(self.keys)
        n_digits = p.base2d().as_1d().size()
        self.addr = pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len()))))
        self.table = bank.table(TABLE_BITS)
        self.table.load(synth(rng, (ws, p.glwe_len())))
        self.rf = bank.regfile(REGS_BITS)
        self.rf.load(synth(rng, (ws, p.glwe_len())))
        digits = {"table": bank.table_selector(TABLE_BITS).n_digits(), "regs": bank.selector(REGS_BITS).n_digits()}
        self.fetch = bank.table_selector(TABLE_BITS, list(synth(rng, (digits["table"], p.ggsw_len()))))
        self.rs = [pkg.Selector.from_digits(bank, REGS_BITS, list(synth(rng, (digits["regs"], p.ggsw_len())))) for _ in range(2)]
        self.rd = pkg.Selector.from_digits(bank, REGS_BITS, list(synth(rng, (digits["regs"], p.ggsw_len()))))
        self.pick = pkg.Selector.from_digits(bank, 1, list(synth(rng, (bank.selector(1).n_digits(), p.ggsw_len()))))
        self.words = synth(rng, (1, ws, p.glwe_len()))
        for what in self.legs():   # once through, so that every buffer a leg grows on first use exists
            self.leg(what)
        return {"lib": pkg.library_path(), "has_rpw_mix": hasattr(pkg.library(), "fheram_bank_read_prepare_write_mix"), "address_digits": n_digits, "selector_digits": digits}

    def legs(self):
        return [w for w, kinds in LEGS.items() if self.kind in kinds]

    def first_halves(self, what):
        bank, keys, a = self.bank, self.keys, self.addr
        lst, tabs, regs = ([0], [a]), ([self.table], [self.fetch]), (self.rf, self.rs)
        if self.kind == "parent":
            if what != "prepare":
                bank.read_mix(list=lst, tables=tabs, regs=regs, download=False)
            bank.read_prepare_write_list([0], [a], keys, download=False)
            self.rf.read_prepare_write(self.rd, download=False)
        elif what == "prepare":
            bank.read_prepare_write_mix(prepare_list=lst, prepare_regs=(self.rf, self.rd), download=False)
        else:
            bank.read_prepare_write_mix(list=None if what == "step5" else lst, tables=tabs, regs=regs, prepare_list=lst, prepare_regs=(self.rf, self.rd), download=False)

    def second_halves(self):
        bank, S = self.bank, self.pkg.Src
        bank.select([self.pick], [[S.member(0), S.host(0)]], host_words=self.words, download=False)
        bank.write_list_selected([0], [0], [self.addr], self.keys)
        self.rf.write(self.rd, S.regs_old())

    def leg(self, what):
        t0 = time.perf_counter()
        self.first_halves(what)
        if what == "whole":
            self.second_halves()
        self.bank.sync()
        dt = time.perf_counter() - t0
        if what != "whole":   # outside the clock: back to state 0
            self.second_halves()
            self.bank.sync()
        return dt

    def profile(self, what):
        """the launches per class of the clocked part, and of the writes behind it"""
        bank = self.bank
        bank.profile_enable(True)
        out = {}
        for part, run in (("first_halves", lambda: self.first_halves(what)), ("second_halves", self.second_halves)):
            bank.profile_reset()
            run()
            bank.sync()
            out[part] = {c: bank.profile_get(c) for c in PROFILE_CLASSES}
        bank.profile_enable(False)
        out["roundoff_max"] = bank.roundoff_max(check=False)
        out["tail_stats"] = bank.tail_stats()
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
    workers = {"parent": MixRemote(args.baseline_lib), "mix": MixRemote(None)}
    result = {"tool": "tools/rpw_mix_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "table_bits": TABLE_BITS, "regs_bits": REGS_BITS,
              "reps": args.reps, "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in one sync",
              "spread": "p10..p90 of the repetitions of a leg over its median",
              "rule": "prepare, step: the mix counts as faster only if it beats the parent leg's median by more than that leg's own spread; "
                      "whole: not slower than its parent leg by more than that spread; step5 is measured against step's parent leg"}
    try:
        info = {k: r.call("setup", kind=k, log_max_addr=args.log_max_addr, ws=args.word_size) for k, r in workers.items()}
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(info["parent"]["lib"], ROOT),
                      candidate_lib=os.path.relpath(info["mix"]["lib"], ROOT), baseline_lib_has_rpw_mix=info["parent"]["has_rpw_mix"],
                      selector_digits=info["mix"]["selector_digits"], address_digits=info["mix"]["address_digits"])
        parent_of = {}
        for what, kinds in LEGS.items():
            for _ in range(args.warmup):
                for k in kinds:
                    workers[k].call("leg", what=what)
            t = {k: [] for k in kinds}
            for _ in range(args.reps):   # alternating: one repetition of each leg in turn
                for k in kinds:
                    t[k].append(workers[k].call("leg", what=what))
            s = {k: summarise(v) for k, v in t.items()}
            if "parent" in s:
                parent_of[what] = s["parent"]
            ref = s.get("parent") or parent_of["step"]
            gain = ref["median_ms"] / s["mix"]["median_ms"]
            row = {"mix_speedup": gain, "saved_ms": ref["median_ms"] - s["mix"]["median_ms"], "parent_spread_rel": ref["spread_rel"],
                   "parent_leg": what if "parent" in s else "step"}
            if what == "whole":
                row["accept_not_slower_than_parent_by_more_than_its_spread"] = bool(gain >= 1.0 - ref["spread_rel"])
            else:
                row["accept_beats_parent_by_more_than_its_spread"] = bool(gain > 1.0 + ref["spread_rel"])
            verdict = [v for k, v in row.items() if k.startswith("accept")][0]
            print(f"2^{args.log_max_addr} {what}: parent {ref['median_ms']:.3f} ms  mix {s['mix']['median_ms']:.3f} ms  gain {gain:.3f}  "
                  f"parent spread {ref['spread_rel']:.3f}  {'met' if verdict else 'NOT met'}", flush=True)
            result[what] = {"ciphertexts": ENTRIES[what] * args.word_size, "legs": s, "against_parent": row,
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
