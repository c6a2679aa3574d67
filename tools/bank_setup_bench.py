#!/usr/bin/env python3
"""Decrypting what a bank leaves on the device: through the host, as the parent commit has to, against the bank's own decrypt calls
(fheram_bank_source_decrypt, fheram_bank_ram_decrypt: k_decrypt_decode).  Word size 4, synthetic normalised limbs, a random ternary secret.

Legs, each in a worker process of its own:
  host   (a) the library named by --baseline-lib (a build of the parent commit): a bank of ONE and a twin Ram context of the same shape
             that holds the secret.  "list": the 4 entries of the last read list downloaded (fheram_bank_read_list_result), decrypted by
             the twin's fheram_glwe_decrypt, decoded on the host (Ram.decrypt_coeff).  "dump": every row of the member downloaded
             (fheram_bank_ram_download), the twin's fheram_glwe_decrypt, the host decode of every data coefficient (vectorised)
  device (b) this tree's library: "list": fheram_bank_source_decrypt of the same 4 entries; "dump": fheram_bank_ram_decrypt of the member

Method as tools/table_bench.py: host clock around calls that end in a sync (every one of these does), the legs alternated repetition by
repetition, the median of --reps repetitions with p10..p90.  Also recorded, from the launch profile: the device time of k_decrypt_decode per
ciphertext in (b), and of k_encrypt_sk<3, 1> (the in-place decrypt of fheram_glwe_decrypt: the same arithmetic without the decode) in (a).
No threshold: nobody has measured these before.

  python tools/bank_setup_bench.py --baseline-lib <parent libfheram.so> --log-max-addr 14 --out profiles/bank_setup_2p14.json
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
ENTRIES = 4


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


class Worker:
    def setup(self, kind, log_max_addr, ws):
        from _pkg import load_package
        pkg = self.pkg = load_package()
        self.kind, self.ws = kind, ws
        p = self.p = pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws)
        rng = np.random.default_rng(4321)
        self.keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * 4 * 2 * N))), synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
        bank = self.bank = pkg.RamBank(p, 1, 0)
        bank.load_encrypted(0, synth(rng, (ws, p.rows(), p.glwe_len())))
        bank._use_keys(self.keys)
        n_digits = p.base2d().as_1d().size()
        addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(ENTRIES)]
        bank.read_list([0] * ENTRIES, addrs, self.keys, download=False)
        bank.sync()
        sk = rng.integers(-1, 2, size=N, dtype=np.int64)
        if kind == "host":
            self.twin = pkg.Ram(p, 0)
            self.dsk = pkg.GLWESecret(self.twin, sk)
        else:
            self.dsk = pkg.GLWESecret(bank, sk)
        self.leg("list")
        self.leg("dump")
        return {"lib": pkg.library_path(), "has_bank_setup": hasattr(pkg.library(), "fheram_bank_source_decrypt"), "rows": p.rows(), "ciphertexts_of_a_dump": ws * p.rows()}

    def host_decode(self, pt):
        """decode_coeff_i64 + rounding of phase limbs [n][3][N] -> values [n][N] (Ram.decrypt_coeff's arithmetic, every coefficient)"""
        p = self.p
        k, b2k = p.k_glwe_ct(), p.basek()
        rem, ls = b2k - (k % b2k), k - p.k_glwe_pt()
        hi = (pt[:, 0] << b2k) + pt[:, 1]
        res = (hi << (b2k - rem)) + (pt[:, 2] >> rem) if rem != b2k else (hi << b2k) + pt[:, 2]
        mag = (np.abs(res) + (1 << (ls - 1))) >> ls if ls > 0 else np.abs(res)
        val = np.where(res < 0, -mag, mag)
        return val, int(np.abs(res - (val << ls)).max())

    def leg(self, what):
        bank, p = self.bank, self.p
        t0 = time.perf_counter()
        if self.kind == "host":
            if what == "list":
                cts = bank.list_result(0, ENTRIES).reshape(-1, p.glwe_len())
                self.twin.decrypt_coeff(self.dsk, cts, [0] * cts.shape[0])
            else:
                rows = bank.store_encrypted(0).reshape(-1, p.glwe_len())
                val, _ = self.host_decode(self.twin.glwe_decrypt(self.dsk, rows))
                np.ascontiguousarray(val.reshape(self.ws, -1).T[:p.max_addr()])   # the interleaved order of the data
        else:
            if what == "list":
                bank.decrypt_sources(self.dsk, [self.pkg.Src.list(k) for k in range(ENTRIES)])
            else:
                bank.decrypt(0, self.dsk)
        return time.perf_counter() - t0

    def profile(self, what):
        owner, cls = (self.twin, "encrypt") if self.kind == "host" else (self.bank, "decrypt_decode")
        owner.profile_enable(True)
        owner.profile_reset()
        self.leg(what)
        got = owner.profile_get(cls)
        owner.profile_enable(False)
        got["kernel"] = "k_encrypt_sk<3, 1>" if self.kind == "host" else "k_decrypt_decode<3>"
        got["us_per_ciphertext"] = got["ms"] * 1e3 / got["blocks"] if got["blocks"] else None
        got["roundoff_max"] = owner.roundoff_max(check=False)
        return got


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
    result = {"tool": "tools/bank_setup_bench.py", "log_max_addr": args.log_max_addr, "word_size": args.word_size, "list_entries": ENTRIES, "reps": args.reps,
              "baseline_is_parent_build": bool(args.baseline_lib), "clock": "host perf_counter around calls that end in a sync",
              "spread": "p10..p90 of the repetitions of a leg over its median"}
    try:
        sb = base.call("setup", kind="host", log_max_addr=args.log_max_addr, ws=args.word_size)
        sc = cand.call("setup", kind="device", log_max_addr=args.log_max_addr, ws=args.word_size)
        result.update(baseline_lib="libfheram.so built from the parent commit" if args.baseline_lib else os.path.relpath(sb["lib"], ROOT),
                      candidate_lib=os.path.relpath(sc["lib"], ROOT), baseline_lib_has_bank_setup=sb["has_bank_setup"], rows=sc["rows"],
                      ciphertexts_of_a_dump=sc["ciphertexts_of_a_dump"])
        legs = [(base, "host"), (cand, "device")]
        for what in ("list", "dump"):
            for _ in range(args.warmup):
                for r, kind in legs:
                    r.call("leg", what=what)
            t = {"host": [], "device": []}
            for _ in range(args.reps):   # alternating: one repetition of each leg in turn
                for r, kind in legs:
                    t[kind].append(r.call("leg", what=what))
            s = {k: summarise(v) for k, v in t.items()}
            gain = s["host"]["median_ms"] / s["device"]["median_ms"]
            result[what] = {"legs": s, "baseline_spread_rel": s["host"]["spread_rel"], "device_speedup_over_host": gain,
                            "saved_ms": s["host"]["median_ms"] - s["device"]["median_ms"],
                            "launch_profile": {kind: r.call("profile", what=what) for r, kind in legs}}
            print(f"2^{args.log_max_addr} {what}: host {s['host']['median_ms']:.3f} ms  device {s['device']['median_ms']:.3f} ms  gain {gain:.2f}  "
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
