"""The sizing of the float-tile Lanczos2 warp's per-launch tables (video_stabilizer_amd/csrc/vs_warp_table.hpp: tile entries, row run padded to
whole 4-row blocks, bytes per frame) against the rule, for the windows of tests/test_warp_tables_gpu.py and every small window, under the
address and undefined-behaviour sanitizers (tests/cpp/warp_table_test.cpp).  Plain host C++: no HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_warp_table_test_%d" % os.getpid()


def test_table_sizing_equals_the_rule_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "warp_table_test.cpp")]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
