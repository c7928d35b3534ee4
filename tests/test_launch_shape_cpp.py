"""The launchers' shared host pieces (video_stabilizer_amd/csrc/vs_launch.hpp: container_ok, for_frame_chunks, rows_on_dwords) against
restatements, under the address and undefined-behaviour sanitizers (tests/cpp/launch_shape_test.cpp: a stand-alone program that checks
itself).  Plain host C++: no HIP, no shared library, nothing preloaded.

What the program asks:
    for_frame_chunks   n in {1, 2, 65535, 65536, 131070, 131071}: the chunks are contiguous, cover [0, n) exactly once, none exceeds 65535
    rows_on_dwords     base offsets 0 .. 7 bytes, element sizes 1 and 2, row strides 1 .. 9, frame strides 0 .. 9, 1 .. 3 frames, 2 rows:
                       yes only where every row of every frame starts on a dword, and exactly where the launchers' former expression
                       ((ptr | stride * esz | (n > 1 ? fs * esz : 0)) & 3) == 0 says yes
    container_ok       bits in {0, 8, 10, 16, 32} x max_value in {-1, 0, 254, 255, 256, 1023, 65535, 65536}: exactly (8, 255) and (16, 0 .. 65535)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_launch_shape_test_%d" % os.getpid()


def test_the_launchers_shared_pieces_against_restatements_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "launch_shape_test.cpp")]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    last = out.stdout.split("\n")[-2].split()
    assert last[0] == "DONE" and int(last[2]) == 0, out.stdout[-500:]
    # 6 chunked lengths, 8 * 2 * 9 * 10 * 3 stride cases with three checks each, 40 containers: the program ran all of it
    assert int(last[1]) >= 3 * 8 * 2 * 9 * 10 * 3 + 40 + 6 * 3, out.stdout[-500:]
