"""CPU: raftsql_amd/csrc/raftq_step_rounds.hpp -- raftq_apply_log_deltas' round planner (which launch each record of a batch belongs
to, and the stable counting sort into launches) -- against a naive model (tests/c/step_rounds_host.cpp: a std::map from group to
count, caller order within a round).  A stand-alone program built with AddressSanitizer + UBSan: every group distinct, one group
named k times, 4,000 seeded random batches on one state, consecutive calls, the epoch's wrap over stale marks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "step_rounds_host.cpp")
HDR = os.path.join(ROOT, "raftsql_amd", "csrc", "raftq_step_rounds.hpp")
EXE = os.path.join(ROOT, "tests", "c", "step_rounds_host")


def _build() -> str:
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.dirname(HDR),
                               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                               "-o", EXE, SRC])
    return EXE


def test_rounds_against_a_naive_model():
    r = subprocess.run([_build()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok:"), r.stdout + r.stderr


def test_the_header_is_host_only():
    """It includes the standard library, nothing of the project's and nothing of HIP: no kernels, no raftq_t."""
    inc = [ln.split()[1] for ln in open(HDR) if ln.startswith("#include")]
    assert inc and all(i.startswith("<") and "hip" not in i for i in inc), inc
