"""THE RESIZE RULE's header (video_stabilizer_amd/csrc/vs_resize.hpp) under the address and undefined-behaviour sanitizers
(tests/cpp/resize_rule_test.cpp, a stand-alone program): every (s, d) up to 512 and the large sizes under both filters -- sums, ranges, tap
counts, both sides of s == 8 d and d == s, the 64-bit products at 32767 -- and the tiled kernel's launch shape: the LDS bound holds for every
shape the tile-rows function admits.  Plain host C++: no HIP, no shared library.  What is checked and the premises the program asserts: its
header comment."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_rule_and_the_launch_shape_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resize_rule_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "resize_rule_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "DONE" and lines[-2].endswith("failures 0"), out.stdout[-500:]
