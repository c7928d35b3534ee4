"""The integer half of the aligner's run path (video_stabilizer_amd/csrc/vs_align_plan.hpp: level table, chunk sizing, frame bookkeeping, the
fused solver's launch plan, result conversion) against the oracle's aligner and against restatements of the rules, under the address and
undefined-behaviour sanitizers (tests/cpp/align_plan_test.cpp).  Plain host C++ together with csrc/vs_host.cpp and the oracle's sources: no
HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_align_plan_test_%d" % os.getpid()


def test_align_plan_equals_the_oracle_and_the_restated_rules_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-march=x86-64-v3", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "align_plan_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp"),
           os.path.join(ROOT, "oracle", "vs_oracle.cpp"), os.path.join(ROOT, "oracle", "vs_phase.cpp"), "-lpthread"]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
