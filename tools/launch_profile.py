#!/usr/bin/env python3
"""Which launches an operation is made of: the launch profile (fheram_profile_get / fheram_bank_profile_get) of a fixed list of operations.

For every size, parameter block and execution form the script runs, on synthetic normalised limbs from fixed seeds,
  a plain context:      read, read_prepare_write, write, a K = 2 and a K = 4 read batch, a second whole step
  banks of M = 2 and 3: read, read_prepare_write, write on the full range, and one step on a single member
and prints one line per operation with every profile class's `launches/blocks` (classes without a launch are left out).  The classes
are the ProfScope names of csrc/launch.hpp and csrc/path.hpp.  They do not tell the column split, the limb split and the fine split of a
single step apart (all are `keyswitch` / `ext_product` with gx * gy blocks); a kernel trace does.

The library named by --lib (default: this tree's) is loaded by a fresh worker process, so two builds are compared by running the script
once per library and comparing the two outputs line by line:

  python tools/launch_profile.py --lib <parent libfheram.so> > parent.txt
  python tools/launch_profile.py > profiles/chain_form_launch_profile.txt
  diff parent.txt profiles/chain_form_launch_profile.txt
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 4096
CLASSES = ["prepare", "ext_product", "ext_product_fused", "ext_product_mid_launch", "keyswitch", "keyswitch_fused", "keyswitch_chain_launch",
           "keyswitch_mid_launch", "keyswitch_tail_launch", "read_chain_launch", "write_chain_launch", "elementwise"]
FORMS = [("default", {}), ("fuse0", {"fuse": 0}), ("tail0", {"tail": 0}), ("tail_ep0", {"tail_ep": 0}), ("mid0", {"mid": 0}),
         ("chain0", {"chain": 0}), ("chain_y0", {"chain_y": 0}), ("limb_split0", {"limb_split": 0})]


def synth(rng, shape):
    return rng.integers(-(1 << 16), 1 << 16, size=shape, dtype=np.int64)


def worker(args):
    from _pkg import load_package
    pkg = load_package()
    pkg.library()
    ws = args.word_size

    def profiled(obj, tag, what, op):
        obj.profile_reset()
        try:
            op()
            obj.sync()
        except pkg.FheRamError as e:   # an operation the library refuses is part of the record
            print(f"{tag} {what:<22} refused: {e}", flush=True)
            return
        got = {c: obj.profile_get(c) for c in CLASSES}
        print(f"{tag} {what:<22}" + "".join(f" {c}={g['launches']}/{g['blocks']}" for c, g in got.items() if g["launches"]), flush=True)

    for log_max_addr in [int(x) for x in args.log_max_addr.split(",")]:
        for block in ("source", "readme"):
            p = (pkg.Parameters(max_addr=1 << log_max_addr, word_size=ws) if block == "source"
                 else pkg.Parameters.readme(max_addr=1 << log_max_addr, word_size=ws))
            s_evk = -(-p.k_evk_trace() // p.basek())
            rng = np.random.default_rng(1234)
            keys = pkg.EvaluationKeysPrepared(pkg.galois_elements(12), list(synth(rng, (12, 3 * s_evk * 2 * N))), synth(rng, 4 * 5 * 2 * N),
                                              synth(rng, 4 * 5 * 2 * N))
            n_digits = p.base2d().as_1d().size()
            addrs = [pkg.Address(p, list(synth(rng, (n_digits, p.ggsw_len())))) for _ in range(4)]
            words = synth(rng, (3, ws, p.glwe_len()))
            rows = [synth(rng, (ws, p.rows(), p.glwe_len())) for _ in range(3)]
            for form, cfg in FORMS:
                tag = f"2^{log_max_addr} {block} {form}"
                ram = pkg.Ram(p, 0, config=cfg)
                ram.load_encrypted(rows[0])
                ram._use_keys(keys)
                ram.profile_enable(True)
                a = addrs[0]

                def step():
                    ram.read(a, keys, download=False)
                    ram.read_prepare_write(a, keys, download=False)
                    ram.write(words[0], a, keys)

                profiled(ram, tag, "read", lambda: ram.read(a, keys, download=False))
                profiled(ram, tag, "read_prepare_write", lambda: ram.read_prepare_write(a, keys, download=False))
                profiled(ram, tag, "write", lambda: ram.write(words[0], a, keys))
                profiled(ram, tag, "batch2", lambda: ram.read_batch(addrs[:2], keys, download=False))
                profiled(ram, tag, "batch4", lambda: ram.read_batch(addrs[:4], keys, download=False))
                profiled(ram, tag, "second step", step)
                ts, ms = ram.tail_stats(), ram.mid_stats()
                print(f"{tag}: context fallbacks tail {ts['fallbacks']}/{ts['launches']} mid {ms['fallbacks']}/{ms['launches']}", file=sys.stderr)
                del ram
                for M in (2, 3):
                    bank = pkg.RamBank(p, M, config=cfg)
                    for m in range(M):
                        bank.load_encrypted(m, rows[m])
                    bank._use_keys(keys)
                    bank.profile_enable(True)
                    am, wm = addrs[:M], words[:M]

                    def member_step():
                        bank.read(am[1:2], keys, first=1, download=False)
                        bank.read_prepare_write(am[1:2], keys, first=1, download=False)
                        bank.write(wm[1:2], am[1:2], keys, first=1)

                    profiled(bank, tag, f"bank{M} read", lambda: bank.read(am, keys, download=False))
                    profiled(bank, tag, f"bank{M} read_prepare_write", lambda: bank.read_prepare_write(am, keys, download=False))
                    profiled(bank, tag, f"bank{M} write", lambda: bank.write(wm, am, keys))
                    profiled(bank, tag, f"bank{M} one-member step", member_step)
                    ts, ms = bank.tail_stats(), bank.mid_stats()
                    print(f"{tag}: bank{M} fallbacks tail {ts['fallbacks']}/{ts['launches']} mid {ms['fallbacks']}/{ms['launches']}", file=sys.stderr)
                    del bank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=None, help="libfheram.so to profile (default: this tree's)")
    ap.add_argument("--log-max-addr", default="12,13,14,16,18")
    ap.add_argument("--word-size", type=int, default=4)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    env = dict(os.environ)
    if args.lib:
        env["FHERAM_LIB"] = os.path.abspath(args.lib)
    else:
        env.pop("FHERAM_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--log-max-addr", args.log_max_addr, "--word-size", str(args.word_size)]
    sys.exit(subprocess.run(cmd, env=env, cwd=ROOT).returncode)


if __name__ == "__main__":
    main()
