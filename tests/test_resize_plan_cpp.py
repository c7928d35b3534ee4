"""What a stabilizer call delivers (video_stabilizer_amd/csrc/vs_stab_plan.hpp: delivered_size -- the crop window, the source frame's size or
the size the handle was given, and whether the resize pass runs) against values worked out by hand, under the address and
undefined-behaviour sanitizers (tests/cpp/resize_plan_test.cpp).  Plain host C++ together with csrc/vs_host.cpp: no HIP, no shared library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_delivered_size_equals_the_hand_worked_table_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resize_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "resize_plan_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
