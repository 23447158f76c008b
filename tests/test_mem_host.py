"""The handle's owning types on the CPU (csrc/pf_mem.h): tests/mem_check.cpp runs them over a counting stand-in for the HIP runtime
and checks the growth rule at its boundaries, a failing allocation, the moves, the lazily created events and streams, the staged
block and the balance of every scenario -- compiled host-only under the address and undefined-behaviour sanitizers and run as a
program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pharmacophore-diffusion_amd", "csrc")
SAN = "-fsanitize=address,undefined -fno-sanitize-recover"


def test_mem_check(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the memory check needs the compiler the library is built with")
    exe = str(tmp_path / "mem_check")
    # pf_mem.h names the runtime's types (hip_runtime_api.h: declarations only, nothing of it is linked or called)
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    cmd = [hipcc, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_inc, "-I" + CSRC]
    cmd += ["-Xarch_host", SAN.split()[0], "-Xarch_host", SAN.split()[1]]
    cmd += [os.path.join(ROOT, "tests", "mem_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "ERROR: LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "mem_check: all checks passed" in r.stdout
