"""The stabilizer's scalar bookkeeping (video_stabilizer_amd/csrc/vs_stab_step.hpp: smoother update, reset of the accumulated correction on a
failed alignment, measurement queue, jitter, decay, correction -- stabilizer.cpp:35-99) against the oracle's extracted step
(oracle/vs_oracle.cpp vso_stabilizer_step), bit for bit after every frame, under the address and undefined-behaviour sanitizers
(tests/cpp/stab_step_test.cpp).  Plain host C++ together with csrc/vs_host.cpp and the oracle's sources: no HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_stab_step_test_%d" % os.getpid()


def test_stabilizer_step_equals_the_oracles_step_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-march=x86-64-v3", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "stab_step_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp"),
           os.path.join(ROOT, "oracle", "vs_oracle.cpp"), os.path.join(ROOT, "oracle", "vs_phase.cpp"), "-lpthread"]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
