"""Compiling the stand-alone host programs of tests/abi/ that evaluate a pure csrc/ header on the CPU
(batch_plan_dump.cpp, meter_sync_dump.cpp): the host compiler against the ROCm headers, or hipcc (a .cpp file
is host code to it) where g++ is missing or cannot digest them."""
import os
import shutil
import subprocess

import pytest


def compile_host_program(src, exe):
    """Builds `src` into `exe`; skips the test where neither compiler is there, fails it where both refuse."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    tried = []
    if shutil.which("g++") and os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        tried.append(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, src])
    if os.path.exists(hipcc):
        tried.append([hipcc, "-std=c++17", "-O1", "-o", exe, src])
    if not tried:
        pytest.skip("neither g++ with the ROCm headers nor hipcc available")
    errs = []
    for cmd in tried:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errs.append(" ".join(cmd) + "\n" + r.stderr[-2000:])
    pytest.fail(os.path.basename(src) + " does not compile:\n" + "\n".join(errs))
