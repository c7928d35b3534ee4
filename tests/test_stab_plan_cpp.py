"""The integer half of the stabilizer's run path (video_stabilizer_amd/csrc/vs_stab_plan.hpp: knob parsing, the route of a call, the depths of
the look-ahead passes, scratch groups, warp runs) and the parameter ranges of vs_internal.hpp, against values worked out by hand from the
former stab_run / stab_chunk and against restated rules, under the address and undefined-behaviour sanitizers
(tests/cpp/stab_plan_test.cpp).  Plain host C++ together with csrc/vs_host.cpp: no HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_stab_plan_test_%d" % os.getpid()


def test_stab_plan_equals_the_hand_worked_table_and_the_restated_rules_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "stab_plan_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
