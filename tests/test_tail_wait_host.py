"""The host side of the tail's done word (fhe-ram_amd/csrc/tail_wait.hpp) without a device: fhe-ram_amd/host/tail_wait_check.cpp is a
stand-alone program that drives the generation comparison, the "last enqueued was the tail and its fallback" bookkeeping and the bounded
poll; built here with the warnings as errors, once plain and once with the address and undefined-behaviour sanitizers, and run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "fhe-ram_amd", "host", "tail_wait_check.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_tail_wait_check_program(tmp_path, flags):
    exe = str(tmp_path / "tail_wait_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, SRC])
    # (the program allocates nothing: the leak checker, which some sandboxes do not let attach, has nothing to find)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip().endswith("tail_wait_check ok"), r.stdout + r.stderr


def test_the_library_uses_that_header():
    """fheram_sync polls through the very struct the program checks, and the enqueue / wait hooks of the context feed it"""
    csrc = os.path.join(ROOT, "fhe-ram_amd", "csrc")
    ctx, lib = open(os.path.join(csrc, "ctx.hpp")).read(), open(os.path.join(csrc, "fheram.hip")).read()
    assert '#include "tail_wait.hpp"' in ctx and "TailWait tail_wait;" in ctx
    assert "c->tail_wait.waited()" in ctx and "c->tail_wait.enqueued()" in ctx
    assert "c->tail_wait.poll()" in lib and lib.count("c->tail_wait.arm()") == 3
