"""The integer rules of the kernel-level C ABI layer (video_stabilizer_amd/csrc/vs_call_plan.hpp: staging capacities, the span rings' placement
and overlap rule, byte spans of batches and image outputs, the window check, CandIndex, frames per launch group, the alignment of the
Lanczos2 tables, the runs of a fill batch) against brute-force restatements, under the address and undefined-behaviour sanitizers
(tests/cpp/call_plan_test.cpp).  Plain host C++: no HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_call_plan_test_%d" % os.getpid()


def test_call_plan_equals_the_restated_rules_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "call_plan_test.cpp")]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
