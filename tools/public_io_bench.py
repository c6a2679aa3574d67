#!/usr/bin/env python3
"""The public side of a bank (fheram_bank_peek / _poke / _ram_load_plain) against what the parent offers for the same job: the
oblivious operations at (trivial) GGSW addresses and the upload of host-built ciphertexts.  Word size 4, synthetic normalised limbs (no
launch depends on a value), a bank of ONE member.

Workers (a process each):
  parent  the library named by --baseline-lib (a build of the parent commit)
  public  this tree's library

Legs (parent form / public form):
  peek1  one word read:      read_list of 1 entry                                      /  peek of 1 entry
  peek8  eight words read:   read_list of 8 entries                                    /  peek of 8 entries
  poke1  one word written:   read_prepare_write_list + write_list                      /  poke of 1 entry
  poke8  eight words of one row written: eight read_prepare_write_list + write_list pairs (a member has one pending write)  /  poke of 8
  load   a whole member:     fheram_bank_ram_upload of a host int64 image built before the clock starts  /  load_plain of the bytes

Method as tools/rpw_mix_bench.py: host clock around calls that end in ONE sync (every call before it has out = NULL), the legs alternated
repetition by repetition, the median of --reps repetitions with p10..p90.

Acceptance: a public leg counts as faster than the parent leg only if it beats that leg's median by more than that leg's
own p10..p90 spread.

  python tools/public_io_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/public_io_2p14.json
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
LEGS = ("peek1", "peek8", "poke1", "poke8", "load")
WORDS = {"peek1": 1, "peek8": 8, "poke1": 1, "poke8": 8}
PROFILE_CLASSES = ("prepare", "ext_product", "keyswitch", "keyswitch_tail_launch", "keyswitch_mid_launch", "keyswitch_chain_launch", "elementwise", "read_chain_launch",
                   "write_chain_launch")


class Worker:
    def setup(self, kind, log_max_addr, ws):
        from _pkg import load_package
        pkg = self.pkg = load_package()
        self.kind = kind
        p = self.p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        rng = np.random.default_rng(4321)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
        bank = self.bank = pkg.RamBank(p, 1, 0)
        self.image = synth(rng, (ws, p.rows(), p.glwe_len()))   # what a host builds from public bytes: [ws][rows][GLWE] int64
        self.bytes = rng.integers(0, 256, size=p.max_addr() * ws, dtype=np.uint8)
        bank.load_encrypted(0, self.image)
        bank._use_keys(self.keys)
        n_digits = p.base2d().as_1d().size()
        self.addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(8)]
        self.public = [(p.max_addr() // 2 // N) * N + 37 * k + 5 for k in range(8)]   # eight words of one row
        self.words = synth(rng, (8, ws, p.glwe_len()))
        for what in LEGS:   # once through, so that every buffer a leg grows on first use exists
            self.leg(what)
        return {"lib": pkg.library_path(), "has_public_side": hasattr(pkg.library(), "fheram_bank_peek"), "address_digits": n_digits, "rows": p.rows(),
                "image_bytes": int(self.image.nbytes), "plain_bytes": int(self.bytes.nbytes)}

    def run(self, what):
        bank, keys = self.bank, self.keys
        if what == "load":
            if self.kind == "parent":
                bank.load_encrypted(0, self.image)
            else:
                bank.load_plain(0, self.bytes)
            return
        n = WORDS[what]
        if self.kind == "parent":
            if what.startswith("peek"):
                bank.read_list([0] * n, self.addrs[:n], keys, download=False)
            else:
                for k in range(n):
                    bank.read_prepare_write_list([0], [self.addrs[k]], keys, download=False)
                    bank.write_list([0], self.words[k:k + 1], [self.addrs[k]], keys)
        elif what.startswith("peek"):
            bank.peek([0] * n, self.public[:n], download=False)
        else:
            bank.poke([0] * n, self.public[:n], words=self.words[:n])

    def leg(self, what):
        t0 = time.perf_counter()
        self.run(what)
        self.bank.sync()
        return time.perf_counter() - t0

    def profile(self, what):
        """the launches per class of the clocked part"""
        bank = self.bank
        bank.profile_enable(True)
        bank.profile_reset()
        self.run(what)
        bank.sync()
        out = {c: bank.profile_get(c) for c in PROFILE_CLASSES}
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


class PublicRemote(Remote):
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
    workers = {"parent": PublicRemote(args.baseline_lib), "public": PublicRemote(None)}
    result = {"tool": "tools/public_io_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "reps": args.reps,
              "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in one sync",
              "spread": "p10..p90 of the repetitions of a leg over its median",
              "rule": "a public leg counts as faster only if it beats the parent leg's median by more than that leg's own spread",
              "note": "synthetic normalised limbs: the parent's addresses stand for trivial GGSW addresses, its image for host-built trivial ciphertexts "
                      "(built before the clock starts)"}
    try:
        info = {k: r.call("setup", kind=k, log_max_addr=args.log_max_addr, ws=args.word_size) for k, r in workers.items()}
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(info["parent"]["lib"], ROOT),
                      candidate_lib=os.path.relpath(info["public"]["lib"], ROOT), baseline_lib_has_public_side=info["parent"]["has_public_side"],
                      address_digits=info["public"]["address_digits"], rows=info["public"]["rows"], image_bytes=info["parent"]["image_bytes"],
                      plain_bytes=info["public"]["plain_bytes"])
        for what in LEGS:
            for _ in range(args.warmup):
                for r in workers.values():
                    r.call("leg", what=what)
            t = {k: [] for k in workers}
            for _ in range(args.reps):   # alternating: one repetition of each leg in turn
                for k, r in workers.items():
                    t[k].append(r.call("leg", what=what))
            s = {k: summarise(v) for k, v in t.items()}
            ref = s["parent"]
            gain = ref["median_ms"] / s["public"]["median_ms"]
            row = {"public_speedup": gain, "saved_ms": ref["median_ms"] - s["public"]["median_ms"], "parent_spread_rel": ref["spread_rel"],
                   "accept_beats_parent_by_more_than_its_spread": bool(gain > 1.0 + ref["spread_rel"])}
            print(f"2^{args.log_max_addr} {what}: parent {ref['median_ms']:.3f} ms  public {s['public']['median_ms']:.3f} ms  gain {gain:.2f}  "
                  f"parent spread {ref['spread_rel']:.3f}  {'met' if row['accept_beats_parent_by_more_than_its_spread'] else 'NOT met'}", flush=True)
            result[what] = {"legs": s, "against_parent": row, "launch_profile": {k: r.call("profile", what=what) for k, r in workers.items()}}
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
