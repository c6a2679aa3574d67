"""fheram_read_batch against K sequential fheram_read on one context (bench.py measures single ops and stays as it is).

Setup: one context at MAX_ADDR = 2^log (default 18), word size 4, synthetic inputs as bench.py makes them (uniform limbs; the timing
does not depend on what the ciphertexts encrypt), K distinct addresses.  For each K: K synchronous reads (each fheram_read followed by
fheram_sync, the reference's calling pattern) against one fheram_read_batch followed by fheram_sync, alternated, >= `reps` repetitions
each after warm-up, host clock around the device synchronisation; the medians are reported.  Results of both are compared once.
Tail / mid launches and fallbacks are recorded over the timed part.

usage: read_batch_bench.py [--log 18] [--ks 1,2,4,8] [--reps 25] [--readme-k 2] [--out FILE]
       read_batch_bench.py --timeline K   (setup, warm-up, then ONE batch of K: for rocprofv3 --kernel-trace)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from _pkg import load_package  # noqa: E402

N = 4096


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


def setup(pkg, log_max_addr, n_addr, crypto):
    s_evk = 5 if crypto else 4
    ram = pkg.Ram.new_from_ram_params(4, [3, 3, 3, 3], 1 << log_max_addr, **crypto)
    p = ram.params
    n_digits = p.base2d().as_1d().size()
    rng = np.random.default_rng(1234)
    keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * s_evk * 2 * N))),
                                      synth(rng, 4 * 5 * 2 * N), synth(rng, 4 * 5 * 2 * N))
    addrs = [pkg.Address(p, list(synth(np.random.default_rng(5000 + j), (n_digits, p.ggsw_len())))) for j in range(n_addr)]
    ram.load_encrypted(synth(np.random.default_rng(4321), (4, ram.local_rows(), p.glwe_len())))
    return ram, keys, addrs


def stats(ram):
    L = ram._lib if hasattr(ram, "_lib") else load_package().library()
    tl, tf, ml, mf = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    L.fheram_tail_stats(ram._h, C.byref(tl), C.byref(tf))
    L.fheram_mid_stats(ram._h, C.byref(ml), C.byref(mf))
    return {"tail_launches": tl.value, "tail_fallbacks": tf.value, "mid_launches": ml.value, "mid_fallbacks": mf.value}


def measure(ram, keys, addrs, k, reps, warmup=5):
    sel = addrs[:k]

    def seq():
        for a in sel:
            ram.read(a, keys, download=False)
            ram.sync()

    def batch():
        ram.read_batch(sel, keys, download=False)
        ram.sync()

    want = np.stack([ram.read(a, keys).copy() for a in sel])
    same = bool(np.array_equal(ram.read_batch(sel, keys), want))
    for _ in range(warmup):
        seq()
        batch()
    s0 = stats(ram)
    ts, tb = [], []
    for _ in range(reps):
        t = time.perf_counter(); seq(); ts.append(time.perf_counter() - t)
        t = time.perf_counter(); batch(); tb.append(time.perf_counter() - t)
    s1 = stats(ram)
    ms_s, ms_b = statistics.median(ts) * 1e3, statistics.median(tb) * 1e3
    return {"k": k, "reps": reps, "sequential_ms": round(ms_s, 4), "batch_ms": round(ms_b, 4), "speedup": round(ms_s / ms_b, 4),
            "sequential_reads_per_s": round(k / ms_s * 1e3, 1), "batch_reads_per_s": round(k / ms_b * 1e3, 1),
            "sequential_ms_min": round(min(ts) * 1e3, 4), "batch_ms_min": round(min(tb) * 1e3, 4),
            "results_equal": same, **{key: s1[key] - s0[key] for key in s0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=18)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--readme-k", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeline", type=int, default=0)
    args = ap.parse_args()
    pkg = load_package()
    ks = [int(x) for x in args.ks.split(",")]
    if args.timeline:
        ram, keys, addrs = setup(pkg, args.log, args.timeline, {})
        for _ in range(5):
            ram.read_batch(addrs, keys, download=False)
            ram.sync()
        ram.read_batch(addrs, keys, download=False)
        ram.sync()
        return
    ram, keys, addrs = setup(pkg, args.log, max(ks), {})
    res = {"max_addr": 1 << args.log, "word_size": 4, "params": "source constants (4-limb trace keys)",
           "device": ram.device_info(), "method": "median of reps, alternated, host clock around fheram_sync; sequential = K x (fheram_read + fheram_sync)",
           "runs": []}
    for k in ks:
        r = measure(ram, keys, addrs, k, args.reps)
        res["runs"].append(r)
        print(json.dumps(r), flush=True)
    del ram
    if args.readme_k:
        ram, keys, addrs = setup(pkg, args.log, args.readme_k, {"k_glwe_pt": 9, "k_evk_trace": 85})
        r = measure(ram, keys, addrs, args.readme_k, args.reps)
        r["params"] = "README block (K_PT = 9, K_EVK = 85: 5-limb trace keys)"
        res["readme"] = r
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
