"""CPU: raftsql_amd/csrc/raftq_buffers.hpp -- the owner of every buffer a handle grows or allocates lazily -- against a fake HIP
runtime (tests/c/buffers_host.cpp: counting fakes over malloc, a switch that makes the k-th call fail).  A stand-alone program
built with AddressSanitizer + UBSan: every kind and sizing rule through grow / fit / regrow / release, every failure point of
a grow and of an all-or-nothing group, the BAR-or-pinned rule both ways; zero live allocations at exit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "buffers_host.cpp")
HDR = os.path.join(ROOT, "raftsql_amd", "csrc", "raftq_buffers.hpp")
EXE = os.path.join(ROOT, "tests", "c", "buffers_host")


def _rocm_include() -> str:
    for cand in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if cand and os.path.exists(os.path.join(cand, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(cand, "include")
    raise RuntimeError("hip_runtime_api.h not found (ROCM_PATH)")


def _build() -> str:
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                               "-I" + _rocm_include(), "-I" + os.path.dirname(HDR), "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", EXE, SRC])
    return EXE


def test_buffers_against_a_fake_runtime():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout + r.stderr


def test_the_header_is_host_only():
    """It includes the runtime's API header and the standard library, nothing of the project's: no kernels, no raftq_t."""
    inc = [ln.split()[1] for ln in open(HDR) if ln.startswith("#include")]
    assert "<hip/hip_runtime_api.h>" in inc
    assert all(i.startswith("<") and (i == "<hip/hip_runtime_api.h>" or "hip" not in i) for i in inc), inc
