"""The look-ahead passes' candidate transforms (video_stabilizer_amd/csrc/vs_lookahead.hpp: what the stabilizer's border fill, deblur, denoise
and deflicker build their lists from) against a restatement of the rule, bit for bit, under the address and undefined-behaviour sanitizers
(tests/cpp/lookahead_test.cpp).  Plain host C++ together with csrc/vs_host.cpp: no HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_lookahead_test_%d" % os.getpid()


def test_lookahead_transforms_equal_the_rule_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "lookahead_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
