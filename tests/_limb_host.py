"""Builds tests/limb_forms_host.cpp — the host build of fhe-ram_amd/csrc/limb_forms_eval.hpp, the text the kernels call — with
the host compiler and -ffp-contract=off: as a shared object for ctypes, or as a stand-alone program (with the sanitizers)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "limb_forms_host.cpp")
FLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "fhe-ram_amd", "csrc")]
SANITIZE = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g"]


def have_compiler():
    return shutil.which("g++") is not None


def build_shared(tmp_dir):
    """-> eval(form, inputs [n][LF_IN]) -> outputs [n][LF_OUT], through the shared object"""
    so = os.path.join(str(tmp_dir), "liblimb_forms_host.so")
    subprocess.check_call(["g++"] + FLAGS + ["-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    fn = lib.limb_forms_eval_host
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]

    def run(form, inputs, n_out_cols=6):
        inputs = np.ascontiguousarray(inputs, dtype=np.float64)
        out = np.zeros((inputs.shape[0], n_out_cols), dtype=np.float64)
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        assert fn(int(form), inputs.shape[0], dp(inputs), dp(out)) == 0
        return out
    return run


def build_program(tmp_dir, sanitize):
    """-> (path of the stand-alone program, whether it carries the sanitizers).  Without the sanitizers' runtime on this
    machine the program is built plain (the caller says so)."""
    exe = os.path.join(str(tmp_dir), "limb_forms_host")
    if sanitize:
        r = subprocess.run(["g++"] + FLAGS + SANITIZE + ["-DLIMB_FORMS_MAIN", "-o", exe, SRC], capture_output=True, text=True)
        if r.returncode == 0:
            return exe, True
        assert "san" in r.stderr, r.stderr      # anything but a missing sanitizer runtime is a build error
    subprocess.check_call(["g++"] + FLAGS + ["-DLIMB_FORMS_MAIN", "-o", exe, SRC])
    return exe, False
