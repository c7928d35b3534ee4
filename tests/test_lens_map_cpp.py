"""The host's lens map (video_stabilizer_amd/csrc/vs_host.cpp: vsi::lens_map_host, what vs_lens_map runs for VS_MEM_HOST) under the address and
undefined-behaviour sanitizers (tests/cpp/lens_map_test.cpp: a filter, one case per line), against the rule's restatement
(tests/_lens_ref.py), bit for bit.  Plain host C++ together with csrc/vs_host.cpp: no HIP, no shared library.

The map lies in a heap block of exactly its extent, so a store in front of pixel (0, 0) or behind the last pixel is the sanitizer's; the row
padding of a pitched map carries a guard value.  The parameters drive positions to NaN (0 * infinity at a vanishing denominator), to
infinity and past the int range: the conversion to int happens behind the saturation, where the undefined-behaviour sanitizer would see one
that does not fit."""
import os
import subprocess

import numpy as np

import _lens_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_lens_map_test_%d" % os.getpid()


def _maps(cases):
    """cases: [(params dict, w, h, map_stride)] -> [(code, map (h, w, 2) or None, changed padding ints)], built and run as
    tests/test_cover_cpp.py does"""
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "lens_map_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    text = "".join("%s %d %d %d\n" % (" ".join(float(p[k]).hex() for k in L.FIELDS), w, h, ms) for p, w, h, ms in cases)
    try:
        out = subprocess.run([EXE], input=text, capture_output=True, text=True, timeout=120)
    finally:
        os.remove(EXE)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    lines = out.stdout.strip().split("\n")
    assert lines[-1] == "DONE %d" % len(cases) and len(lines) == len(cases) + 1, out.stdout[-500:]
    res = []
    for (p, w, h, ms), ln in zip(cases, lines):
        f = ln.split()
        if f[0] != "0":
            res.append((int(f[0]), None, 0))
            continue
        assert f[-2] == "pad" and len(f) == 2 * w * h + 3
        res.append((0, np.array(f[1:-2], np.int64).reshape(h, w, 2), int(f[-1])))
    return res


def test_the_host_map_under_sanitizers():
    INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
    cases = []
    for w, h, ms in ((1, 1, 2), (2, 3, 4), (2, 3, 9), (96, 64, 2 * 96 + 5), (33, 2, 70)):
        for kw in (dict(), dict(k1=-0.25, k2=0.05, p1=0.001, p2=-0.002), dict(k1=-0.3, k2=0.1, k3=-0.01, k4=0.01, k5=0.02, k6=-0.003),
                   dict(k1=0.1, k4=-5.0), dict(k1=0.2, zoom=1.3, cx=10.25, cy=-3.5)):
            cases.append((L.params(w, h, **kw), w, h, ms))
    w, h, ms = 5, 4, 13
    hostile = [dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, k4=-1.0),                      # the denominator is exactly 0 at r2 == 1: x * inf, 0 * inf
               dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=-1.0, k4=-1.0),             # 0 / 0 there
               dict(fx=1e300, fy=1e-300, k1=1e300),                                # products that overflow to infinity
               dict(fx=1.0, fy=1.0, cx=1e308, cy=-1e308, k3=1e308),                # infinity - infinity
               dict(fx=1e-3, fy=1e-3, k1=1e9, k2=-1e12),                           # finite positions far past the int range, both signs
               dict(fx=4e7, fy=4e7, cx=6.7e7, cy=-6.7e7),                          # positions right at the int range's ends
               dict(k1=1e-320, zoom=5e-324, fx=5e-324)]                            # subnormal parameters: fx * zoom underflows to 0, x is an infinity
    first_hostile = len(cases)
    for kw in hostile:
        cases.append((L.params(w, h, **kw), w, h, ms))
    refused = [(L.params(4, 4, k1=float("nan")), 4, 4, 8), (L.params(4, 4, zoom=float("inf")), 4, 4, 8), (L.params(4, 4, fx=0.0), 4, 4, 8),
               (L.params(4, 4), 4, 4, 7), (L.params(4, 4), 0, 4, 8), (L.params(4, 4), 4, 32768, 8)]
    cases += refused
    got = _maps(cases)
    seen = set()
    for (p, cw, ch, cms), (code, m, changed) in zip(cases[:-len(refused)], got):
        want = L.lens_map(p, cw, ch)
        assert code == 0 and changed == 0
        assert np.array_equal(m, want), (cw, ch, cms, {k: float(v) for k, v in p.items()})
        seen |= set(np.unique(m[(m == INT_MIN) | (m == INT_MAX) | (m == 0)]).tolist())
    assert {INT_MIN, INT_MAX, 0} <= seen                             # the hostile cases did saturate both ways
    nan_case = got[first_hostile + 1][1]
    assert tuple(nan_case[0, 1]) == (0, 0)                           # NaN -> 0
    for code, m, _ in got[-len(refused):]:
        assert code == -1 and m is None
