"""The GPU-free pieces of the whole-solve kernel's speculative cost route
(csrc/dilqr_cost_check.h: the record test and the schedule of the records over
the iterations' steps) are plain C++ on the host.  tests/host/cost_check_host.cpp
enumerates T in 1..40 x iterations in 1..12 x spread in 0..12 x waves and checks
that every record 1 .. T-2 is issued and tested exactly once, in order, inside
the planned iterations, with the drain taking exactly the rest; it is built as a
stand-alone program with AddressSanitizer and UBSan, their runtimes linked in
statically, and run here; a g++ without those runtimes fails the test."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "cost_check_host.cpp")
CSRC = os.path.join(ROOT, "differentiable-ilqr_amd", "csrc")


def test_cost_check_schedule_and_record_test_on_host(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ not found"
    exe = str(tmp_path / "cost_check_host")
    base = [gxx, "-std=c++17", "-O1", "-g", "-I", CSRC, SRC, "-o", exe]
    # the sanitizer runtimes linked into the program itself: it runs whatever
    # else the environment loads into a process first
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(base + san, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.startswith("ok:"), run.stdout
