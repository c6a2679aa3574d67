"""bench.py's other modes on the one GPU of the test box: the external-product microbenchmark
(BASELINE.json configs[1]) and the row-sharded path with ONE rank under torch.distributed.run — RCCL
all-gather / broadcast on device int32 buffers, ordered against the evaluator's stream with events
(fheram_stream_signal / fheram_stream_wait), i.e. exactly the code N > 1 ranks run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def last_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout[-2000:]
    return json.loads(lines[-1])


def test_bench_external_product_mode():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "ep", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = last_json(r.stdout)
    assert out["value"] > 0 and 1.0 < out["latency_us_single_product"] < 200.0
    assert out["roofline"]["bound"] == "valu_fp64" and 0.0 < out["roofline"]["frac"] < 1.0 and 0.0 < out["roofline_hbm"]["frac"] < 1.0


def test_bench_plain_run_dumps_the_last_step(tmp_path, po):
    """A plain run (no --full) prints the headline line only; --dump-outputs writes what its last timed step returned, the same
    from run to run, and equal to the oracle driven through the same warm-up + timed steps on the same inputs."""
    import numpy as np
    import bench
    from _pkg import load_package
    log_max_addr, ws, warmup, steps = 13, 4, 1, 2
    names = ("read", "read_prepare_write", "rows_after_write")
    dumps = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--log-max-addr", str(log_max_addr), "--steps", str(steps),
                            "--warmup", str(warmup), "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = last_json(r.stdout)
        assert out["steps"] == steps and out["value"] > 0 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
        assert out["dtype"] == "f64" and out["unit"].startswith("RAM ops/s")
        assert not any(k in out for k in ("read_ms", "roofline", "cpu_baseline", "parity_in_run", "reference_published"))
        assert sorted(os.listdir(tmp_path / run)) == sorted(n + ".npy" for n in names)
        dumps.append({n: np.load(tmp_path / run / (n + ".npy")) for n in names})
    for n in names:
        assert dumps[0][n].dtype == np.float64 and np.array_equal(dumps[0][n], dumps[1][n]), n

    p = load_package().Parameters(max_addr=1 << log_max_addr, word_size=ws)
    inp = bench.make_inputs(p, ws, 4, p.base2d().as_1d().size(), p.rows())
    o = po.Oracle(po.OParams(max_addr=1 << log_max_addr, word_size=ws))
    keys = o.keys_prepare({"gal_els": np.array([int(po.lib().fo_galois_element(12, i)) for i in range(12)], dtype=np.int64),
                           "atk_glwe": inp["atk"], "atk_ggsw_inv": inp["atk_inv"], "tsk": inp["tsk"]})
    addr = o.address_new(inp["addr"])
    ram = o.ram_new()
    ram.load(inp["rows"])
    for _ in range(warmup + steps):
        want = {"read": ram.read(addr, keys), "read_prepare_write": ram.read_prepare_write(addr, keys)}
        ram.write(inp["words"], addr, keys)
    want["rows_after_write"] = ram.store()
    for n in names:
        assert dumps[0][n].shape == want[n].shape and np.array_equal(dumps[0][n], want[n].astype(np.float64)), n


def test_bench_sharded_one_rank_rccl_device_buffers():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", "29553", os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--mode", "sharded", "--log-max-addr", "14", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-kernel-timing"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = last_json(r.stdout)
    assert out["mode"] == "sharded" and out["value"] > 0


def test_bench_sharded_two_ranks_gloo_on_one_gpu():
    """N = 2 ranks of bench.py's default mode (ONE RAM sharded over the ranks), rehearsed on the one GPU with gloo and
    host exchange buffers: weak scaling (2^13 entries per rank) and strong scaling (--total-log-max-addr 14)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for extra, scaling in (([], "weak"), (["--total-log-max-addr", "14"], "strong")):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                            "--master-addr", "127.0.0.1", "--master-port", "29557", os.path.join(ROOT, "bench.py"),
                            "--gpus", "2", "--dist-backend", "gloo", "--all-ranks-device0", "--log-max-addr", "13",
                            "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-kernel-timing"] + extra,
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out = last_json(r.stdout)
        assert out["mode"] == "sharded" and out["n_gpus"] == 2 and out["scaling"] == scaling and out["value"] > 0
        assert "MAX_ADDR=2^14" in out["config"]["workload"]


def test_bench_starts_its_own_ranks_when_no_launcher_is_around():
    """`python bench.py --gpus 2` WITHOUT torch.distributed.run (how the driver calls it): bench.py starts the two ranks
    itself as child processes — never a silent 1-GPU run."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--all-ranks-device0",
                        "--log-max-addr", "13", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-kernel-timing"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = last_json(r.stdout)
    assert out["n_gpus"] == 2 and out["mode"] == "sharded" and out["value"] > 0
    # a launcher environment that contradicts --gpus is refused, not silently reinterpreted
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(env, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert r.returncode != 0 and "refusing" in (r.stdout + r.stderr)


def test_bench_native_group_mode_on_one_gpu():
    """--mode group: one process drives the sharded RAM through fheram_group_* (here 2 shards on GPU 0)"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--mode", "group", "--all-ranks-device0",
                        "--log-max-addr", "13", "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = last_json(r.stdout)
    assert out["mode"] == "group" and out["n_gpus"] == 2 and out["value"] > 0 and "MAX_ADDR=2^14" in out["config"]["workload"]


def test_scale_check_rehearsal_on_one_gpu():
    """tools/scale_check.sh — the one command for the first contact with an 8-GPU node (digests through the native group and
    through one process per GPU, then bench.py in both modes, N = 1/2/4/8) — rehearsed on the one GPU of the test box: every
    shard on device 0, gloo instead of RCCL, the 2^18 digests (the 2^21 ones through 8 shards: test_gpu_golden.py), the
    process-per-GPU legs up to N = 4 (the box admits 6 GPU processes)."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "scale_check.sh")],
                       env=dict(os.environ, REHEARSE="1", LOG="18", STEPS="2", WARM="1", RANKS_MAX="4"), capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "every digest reproduced at every N" in r.stdout
    lines = [l for l in r.stdout.splitlines() if l[:1].isdigit()]
    assert len(lines) == 4 + 3 and all("FAILED" not in l for l in lines), r.stdout
