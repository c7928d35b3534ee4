"""The host's "candidate 0 covers the whole window" (video_stabilizer_amd/csrc/vs_lookahead.hpp: vsi::cv_window_covered -- the decision that
lets the stabilizer's inpaint skip a whole run) against the rule (tests/_fill_ref.py: covered(), pixel by pixel), under the address and
undefined-behaviour sanitizers (tests/cpp/cover_test.cpp: a filter, one case per line).  Plain host C++ together with csrc/vs_host.cpp: no
HIP, no shared library.

What is asked of every case, with `small` = every table term of the window's rows and columns is below 2^29 in magnitude:
    decision => every pixel of the window is covered        (always: a wrong "yes" leaves black slivers in the output)
    small    => decision == every pixel is covered          (monotone terms: the corners decide)
    not small => decision is 0                               (the sums could wrap: the pass runs and the kernels decide pixel by pixel)"""
import os
import subprocess

import numpy as np

import _fill_ref as RF
import _hostile_maps as HM
import _inpaint_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_cover_test_%d" % os.getpid()


def _decisions(cases):
    """cases: [(transform tuple, w, h, (rx, ry, rw, rh))] -> [0 / 1] from the program, built and run as tests/test_lookahead_cpp.py does"""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "cover_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    text = "".join("%s %s %s %s %d %d %d %d %d %d\n" % (*(float(v).hex() for v in t), w, h, *roi) for t, w, h, roi in cases)
    try:
        out = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.split()
    assert lines[-2:] == ["DONE", str(len(cases))] and len(lines) == len(cases) + 2, out.stdout[-500:]
    assert set(lines[:-2]) <= {"0", "1"}
    return [int(v) for v in lines[:-2]]


def _hostile_cases(O, w, h):
    maps = dict(HM.HOSTILE)
    maps.update(HM.FILL_EXTREME)
    maps["row0_trap"] = HM.row0_trap(O, w, h)
    windows = [(0, 0, w, h), (0, 0, w, 1), (3, 0, 33, 1), (0, 0, 1, h), (5, 7, 20, 11), (w - 1, h - 1, 1, 1), (1, 1, w - 2, h - 2)]
    return [("%s %s" % (name, roi), maps[name], roi) for name in sorted(maps) for roi in windows]


def _random_cases(w, h, n):
    rng = np.random.default_rng(2024)
    out = []
    for i in range(n):
        z, a = rng.uniform(0.9, 1.6), rng.uniform(-0.1, 0.1)
        t = (z * np.cos(a) - 1, z * np.sin(a), rng.uniform(-6, 6), rng.uniform(-6, 6))
        rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        out.append(("random %d" % i, t, (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh)))
    return out


def test_the_host_rectangle_test_against_the_rule_under_sanitizers(oracle):
    O = oracle
    w, h = 64, 48
    hostile, rnd = _hostile_cases(O, w, h), _random_cases(w, h, 3000)
    assert len(hostile) == 30 * 7
    cases = [(name, t, w, h, roi) for name, t, roi in hostile + rnd]
    # a 1920 x 1080 frame with the crop's margins on all four sides, camera jitter from a pixel to more than the margin
    rng = np.random.default_rng(7)
    for crop in (32, 5):
        for i in range(20):
            amp = (1, 4, 16, 40)[i % 4]
            t = (rng.uniform(-0.004, 0.004), rng.uniform(-0.004, 0.004), rng.uniform(-amp, amp), rng.uniform(-amp, amp))
            cases.append(("1080p crop %d jitter %d" % (crop, i), t, 1920, 1080, (crop, crop, 1920 - 2 * crop, 1080 - 2 * crop)))
    # the largest frame the passes take, small windows near the far corner: short of the last column and row, and on them
    big = 32767
    for name, t in (("identity", (0.0, 0.0, 0.0, 0.0)), ("shift in", (0.0, 0.0, 3.0, 2.5)), ("shift out", (0.0, 0.0, -3.0, -2.5)), ("zoom", (0.01, 0.0, 0.0, 0.0)),
                    ("shrink", (-0.001, 0.0, 0.0, 0.0)), ("turn", (0.0, 1e-4, 0.0, 0.0))):
        cases.append(("32767 inner " + name, t, big, big, (big - 41, big - 51, 40, 50)))
        cases.append(("32767 corner " + name, t, big, big, (big - 40, big - 50, 40, 50)))
    want, small = [], []
    with np.errstate(all="ignore"):
        for name, t, fw, fh, roi in cases:
            tt = O.Transform.of(*t)
            cov, sm = IC.covered_window(O, tt, fw, fh, roi)
            if (fw, fh) == (w, h):                                   # the rule itself, full frame, cropped
                x, y, rw, rh = roi
                assert np.array_equal(cov, RF.covered(O, tt, fw, fh)[y:y + rh, x:x + rw]), name
            want.append(bool(cov.all()))
            small.append(sm)
    # premises: both decisions occur among the random cases, among the 1080p ones and among the 32767 ones; some hostile case is not small
    n_h, n_r = len(hostile), len(rnd)
    assert 0.05 * n_r < sum(want[n_h:n_h + n_r]) < 0.95 * n_r
    assert 0 < sum(want[n_h + n_r:n_h + n_r + 40]) < 40 and 0 < sum(want[n_h + n_r + 40:]) < 12
    assert sum(not s for s in small[:n_h]) >= 20 and all(small[n_h:])
    got = _decisions([c[1:] for c in cases])
    unsound = [c[0] for c, g, wnt in zip(cases, got, want) if g and not wnt]
    inexact = [c[0] for c, g, wnt, sm in zip(cases, got, want, small) if sm and bool(g) != wnt]
    not_refused = [c[0] for c, g, sm in zip(cases, got, small) if not sm and g]
    print("%d cases: %d yes, %d no, %d not small; %d unsound, %d inexact" % (len(cases), sum(got), len(got) - sum(got), sum(not s for s in small),
                                                                           len(unsound), len(inexact)))
    assert not unsound, ("'covered' where the rule leaves a pixel open", unsound[:10])
    assert not inexact, ("small terms, yet the decision is not the rule's", inexact[:10])
    assert not not_refused, ("a term of 2^29 or more, yet 'covered'", not_refused[:10])
