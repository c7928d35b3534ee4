"""The tile-window decision of the float-tile warps (video_stabilizer_amd/csrc/vs_c3_window.hpp: vsd::c3_tile_window, the one copy that both
geometry paths of vs_k_bgr_warp_c3 and vs_k_warp_c3_tables call; c3_extents, c3_compact_shape) against the sampler's own positions, pixel by
pixel, under the address and undefined-behaviour sanitizers (tests/cpp/c3_window_test.cpp: a stand-alone program).  Plain host C++ together
with csrc/vs_host.cpp, -ffp-contract=off as the library is built: no HIP, no shared library.

What the program's grid asks of every tile, for every instantiation's (staged rows, column groups, pitch) -- 24 x 20 x 81, 20 x 20 x 81,
20 x 18 x 73 and the raw tiles' 40 x 20 x 88 and 24 x 20 x 88 -- with the frame's extents and from the four corners:
    SOUND    fits => the whole tap window of every live pixel lies inside the staged window, positions formed in the sampler's plain and in
             its tabled order of operations
    EXACT    fits => the sampler's fp32 tile offset (place() of vs_warp.hip, restated) equals the integer offset for every pixel
    REFUSED  fits => the window is not larger than the instantiation's; a footprint at 10^6 or beyond never fits
    COMPACT  c3_compact_shape admits a frame to the 20-row shapes only where every tile's footprint has at most 20 rows (18 groups for shape 2)
    PREMISE  the form this replaced (kept in the program only: fits by magnitude and extent alone) is INEXACT on every far-row case -- identity
             scale, columns inside the frame, rows beyond 2^24 / pitch -- of every instantiation: the grid reaches the fault the guard is for.
The grid: identity, turns of 0.2 to 90 degrees, zooms 0.5 to 2, mirrors, singular and near-singular maps; shifts 0, +-1e4, +-1.9e5 .. +-2.4e5
in steps of 5000 (they straddle 2^24 / 88, / 81 and / 73), +-3e5, +-9.9e5 and both sides of 1e6, in x, in y and in both; whole windows and
windows at odd offsets, every tile of them.

Then the program's decisions on a list of cases are compared with the numpy restatement of tests/_warp_c3_cases.py, which the GPU suite's
builders assert their premises with: premises about the restatement are premises about the real function."""
import os
import re
import subprocess

import numpy as np
import pytest

import _warp_c3_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = "/tmp/vs_c3_window_test_%d" % os.getpid()


@pytest.fixture(scope="module")
def exe():
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", EXE,
           os.path.join(ROOT, "tests", "cpp", "c3_window_test.cpp"), os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_host.cpp")]
    subprocess.check_call(cmd)
    yield EXE
    os.remove(EXE)


def _clean(out):
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]


def test_the_tile_window_decision_against_the_sampler_s_positions_under_sanitizers(exe):
    out = subprocess.run([exe, "grid"], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    _clean(out)
    lines = out.stdout.splitlines()
    assert lines[-1] == "DONE", out.stdout[-2000:]
    assert out.returncode == 0 and not [ln for ln in lines if ln.startswith("BAD")], out.stdout[-3000:]
    seen = {}
    for ln in lines:
        m = re.match(r"(\S+) tiles (\d+) fits (\d+) \| new unsound (\d+) inexact (\d+) oversized (\d+) \| old fits (\d+) unsound (\d+) inexact (\d+) "
                     r"far_row_cases (\d+) far_row_inexact (\d+)$", ln)
        if m:
            seen[m.group(1)] = [int(v) for v in m.groups()[1:]]
    assert sorted(seen) == sorted(s[0] for s in WC.SHAPES)
    for name, (tiles, fits, unsound, inexact, oversized, old_fits, old_unsound, old_inexact, far_cases, far_inexact) in seen.items():
        assert tiles > 30000 and 0.2 * tiles < fits < 0.8 * tiles, (name, tiles, fits)
        assert unsound == 0 and inexact == 0 and oversized == 0, (name, unsound, inexact, oversized)
        # the replaced form: sound -- the footprint was never the fault -- and inexact on EVERY far-row case of this pitch
        assert old_unsound == 0 and old_fits > fits, (name, old_unsound, old_fits)
        assert far_cases >= 24 and far_inexact == far_cases and old_inexact >= far_cases, (name, far_cases, far_inexact, old_inexact)
    m = re.search(r"COMPACT checked (\d+) bad (\d+)", out.stdout)
    assert m and int(m.group(1)) > 10000 and int(m.group(2)) == 0, m


def _cases():
    """(transform, w, h, roi, shape, with_extents): the GPU suite's maps on three windows, its fit sweep on its own"""
    out = []
    w, h = 130, 70
    for name, t in sorted(WC.hostile_maps(w, h).items()):
        for roi in ((0, 0, w, h), (5, 7, 21, 11), (1, 3, w - 1, 33)):
            out += [(t, w, h, roi, k, we) for k in range(len(WC.SHAPES)) for we in (0, 1)]
    sw, sh = WC.SWEEP_SHAPE
    for name, t in WC.fit_sweep():
        for roi in WC.SWEEP_WINDOWS:
            out += [(t, sw, sh, roi, k, we) for k in range(len(WC.SHAPES)) for we in (0, 1)]
    for t in WC.far_rows().values():                                  # the one-row frame and the tiny frames of the route tests
        out += [(t, 200, 1, (0, 0, 200, 1), k, we) for k in range(len(WC.SHAPES)) for we in (0, 1)]
        out += [(t, 67, 21, (0, 0, 67, 21), k, we) for k in range(len(WC.SHAPES)) for we in (0, 1)]
    return out


def test_the_numpy_restatement_takes_the_program_s_decisions(exe):
    cases = _cases()
    text = "".join("%s %s %s %s %d %d %d %d %d %d %d %d\n" % (*(float(v).hex() for v in t), w, h, *roi, k, we) for t, w, h, roi, k, we in cases)
    out = subprocess.run([exe, "cases"], input=text, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    _clean(out)
    lines = out.stdout.splitlines()
    assert lines[-1] == "DONE %d" % len(cases), out.stdout[-500:]
    it = iter(lines[:-1])
    n_tiles = n_fits = n_guard = 0
    shapes_seen = set()
    for t, w, h, roi, k, we in cases:
        head = next(it).split()
        assert head[0] == "E"
        E, compact, tiles = WC.decisions(t, w, h, roi, k, bool(we))
        assert [float.fromhex(v) for v in head[1:5]] == [float(v) for v in E] and int(head[5]) == compact, (t, roi, k, head, E, compact)
        shapes_seen.add(compact)
        for want in tiles:
            got = [int(v) for v in next(it).split()]
            assert got == [int(v) for v in want], (t, w, h, roi, WC.SHAPES[k][0], we, got, want)
            n_tiles += 1
            n_fits += got[2]
            n_guard += (not got[2]) and 0 < got[5] <= WC.SHAPES[k][2] and 0 < got[6] <= WC.SHAPES[k][3]
        assert next(it) == "END %d" % len(tiles)
    print("%d cases, %d tiles: %d fit, %d refused by the offset guard alone" % (len(cases), n_tiles, n_fits, n_guard))
    assert shapes_seen == {0, 1, 2} and n_guard > 1000 and 0.2 * n_tiles < n_fits < 0.9 * n_tiles


def test_the_fit_sweep_meets_every_limit_and_both_sides_of_the_thresholds():
    WC.sweep_premises()
