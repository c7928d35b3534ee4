"""The YCbCr rule's header (video_stabilizer_amd/csrc/vs_ycbcr.hpp) against apps/video_io.hpp under the address and undefined-behaviour
sanitizers (tests/cpp/ycbcr_rule_test.cpp, a stand-alone program): every 8-bit triple and millions of deeper ones through the per-pixel
functions, whole frames of every y4m layout through small files.  Plain host C++: no HIP, no shared library.  What is compared and the premises
the program asserts: its header comment."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rule_equals_video_io_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ycbcr_rule_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "ycbcr_rule_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "DONE" and lines[-2].endswith("frames 32 mismatches 0"), out.stdout[-500:]
