"""The stabilizer's step with scene cuts (video_stabilizer_amd/csrc/vs_stab_step.hpp: stab_step_cut) against stab_step, bit for bit, over random
sequences without a cut (failed alignments and non-finite measurements included), and on hand-worked sequences with a cut at lag 0, 1 and 4: accum
untouched until the cut frame is finalised, the identity then, ok 0 at the cut -- under the address and undefined-behaviour sanitizers
(tests/cpp/scene_step_test.cpp).  Plain host C++ together with csrc/vs_host.cpp: no HIP, no shared library.  The restatement of the same step in
Python (tests/_scene_ref.py: Step) is held against the program's rule here too, on the hand-worked sequence."""
import os
import subprocess

import _scene_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_scene_step_test_%d" % os.getpid()


def test_step_with_cuts_under_sanitizers():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-march=x86-64-v3", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", EXE, os.path.join(ROOT, "tests", "cpp", "scene_step_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    try:
        out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL PASS" in out.stdout.splitlines(), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr


def test_python_step_on_the_hand_worked_sequence(vs):
    """smoother off, lag 1, translations of 10 along x, a cut at frame 3: accum is 0.9 * (accum + 10) frame after frame, the identity when the cut
    frame is finalised (by frame 4), and 9 again after it"""
    p = vs.stabilizer_params(lag=1, enable_smoother=0, smoother_memory=2)
    st = R.Step(vs, p, 320, 240)
    m = vs.Transform.of(0, 0, 10, 0)
    want, seen = 0.0, []
    for i in range(6):
        corr = st.step(m, True, i == 3)
        assert (corr is not None) == (i >= 1)
        if i >= 1:
            want = 0.0 if i - 1 == 3 else (want + 10.0) * p.min_decay
        assert st.accum.tup() == (0.0, 0.0, want, 0.0)
        seen.append(want)
        if i == 3:
            assert st.ok[-1] == 0 and st.meas[-1].tup() == (0.0, 0.0, 0.0, 0.0)
        if i == 4:
            assert corr.tup() == vs.t_inverse(vs.Transform.of()).tup() and vs.t_max_corner_displacement(corr, 320, 240) == 0.0
    assert seen[3] > 20 and seen[4] == 0.0 and seen[5] == 10.0 * p.min_decay
