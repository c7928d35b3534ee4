"""The sharpen pass on the GPU (include/vs_amd.h: vs_bgr_sharpen_batch) against the rule's restatement (tests/_sharpen_ref.py): np.array_equal --
the rule fixes every bit.  Every case asserts its premise on the restatement before it looks at the GPU."""
import numpy as np
import pytest

import _sharpen_ref as R

pytestmark = pytest.mark.gpu

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr16": (4, np.uint16, 16)}
# (roi_w, roi_h).  1 x 1, 2 x 2: no eligible pixel; 3 x 3: one; 4 x 3: the smallest window of the four-pixels-per-lane kernel; 255 / 256 / 257 / 260
# columns: the wave's column seam in both kernels (256 and 260: four pixels a lane, a wave is 256 columns; 255 and 257: one pixel a lane, waves of 64);
# 9 rows: one past a wave's strip of 8; 33 rows: one past a workgroup's four strips
WINDOWS = [(1, 1), (2, 2), (3, 3), (4, 3), (5, 5), (255, 5), (256, 5), (257, 5), (260, 5), (12, 9), (7, 9), (8, 33), (67, 33)]
ORIGINS = [(0, 0), (3, 5)]                                               # ROI origins 0 and odd


def _maps(vs, w, h):
    """identity; a whole-pixel shift; half-pixel shifts; a rotation with zoom; a shrinking rotation, whose source covers a tilted rectangle in the
    middle of the frame (uncovered neighbours on all four sides); a shift with rotation that leaves a corner uncovered"""
    T = vs.Transform.of
    return [T(), T(0, 0, 2, -1), T(0, 0, 0.5, 0.5), T(0, 0, -0.5, 0), T(0.03, 0.05, 1.25, -0.75), T(-0.25, 0.12, 0.4, -0.3), T(0.01, 0.04, 0.22 * w, 0.3 * h)]


def _noise(rng, n, h, w, dtype, maxv):
    return rng.integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)


def _ring_sides(V, t, w, h, roi):
    """how many interior covered pixels of the window lose their eligibility to an uncovered (left, right, upper, lower) neighbour"""
    X, Y = R.positions(V, t, w, h)
    x, y, rw, rh = roi
    cov = R.covered(X, Y, w, h)[y:y + rh, x:x + rw]
    if rw < 3 or rh < 3:
        return np.zeros(4, np.int64)
    c = cov[1:-1, 1:-1]
    return np.array([(c & ~cov[1:-1, :-2]).sum(), (c & ~cov[1:-1, 2:]).sum(), (c & ~cov[:-2, 1:-1]).sum(), (c & ~cov[2:, 1:-1]).sum()])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_windows_origins_and_maps_equal_the_rule(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(300 + bits)
    changed = 0
    sides = np.zeros(4, np.int64)
    for rw, rh in WINDOWS:
        for rx, ry in ORIGINS:
            w, h = rx + rw + (rx and 2), ry + rh + (ry and 4)            # (origin 0: the window is the frame; else a margin on every side)
            roi = (rx, ry, rw, rh)
            ts = _maps(vs, w, h)
            src = _noise(rng, len(ts), rh, rw, dtype, maxv)
            want = R.batch(vs, src, ts, w, h, roi, 16, maxv)
            assert np.array_equal(want[:2], src[:2])                     # premise: the identity and the whole-pixel shift change nothing
            changed += int((want != src).sum())
            for t in ts:
                sides += _ring_sides(vs, t, w, h, roi)
            got = vs.sharpen_batch(src, ts, w, h, rx, ry, fmt=code)      # NULL parameters: strength 16
            assert np.array_equal(got, want), (rw, rh, rx, ry, np.argwhere(got != want)[:5].tolist())
    assert changed > 20000 and (sides > 200).all(), (changed, sides)    # the comparison was about changed pixels, and about the ring on all four sides


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_pitched_rows_and_strengths(gpu_vs, fmt):
    """rows that keep every dword alignment (pitch + 8 elements), rows that lose it (pitch + 7: the sample-by-sample kernel also where the width is
    a multiple of 4), either side alone; the destination's padding stays as it was.  Strengths 1, 16, 32"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(400 + bits)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    for (rw, rh), (rx, ry) in (((260, 9), (0, 0)), ((64, 10), (3, 5)), ((13, 9), (1, 1))):
        w, h = rx + rw + 3, ry + rh + 2
        ts = _maps(vs, w, h)
        src = _noise(rng, len(ts), rh, rw, dtype, maxv)
        for s in (1, 16, 32):
            want = R.batch(vs, src, ts, w, h, (rx, ry, rw, rh), s, maxv)
            assert (want != src).any()
            for ss, ds in ((3 * rw + 8, 3 * rw + 8), (3 * rw + 7, 3 * rw + 7), (3 * rw + 7, 3 * rw), (3 * rw, 3 * rw + 5)):
                got, buf = vs.sharpen_batch(src, ts, w, h, rx, ry, params=vs.sharpen_params(strength=s), fmt=code, src_stride=ss, dst_stride=ds, guard=guard)
                assert np.array_equal(got, want), (rw, rh, s, ss, ds)
                assert (buf[:, :, 3 * rw:] == guard).all()


@pytest.mark.parametrize("n", [0, 1, 70])
def test_frame_counts(gpu_vs, n):
    """70 frames of 12 x 9: more matrices than a kernel-argument block carries"""
    vs = gpu_vs
    rng = np.random.default_rng(70 + n)
    w, h = 16, 13
    roi = (1, 2, 12, 9)
    src = _noise(rng, n, 9, 12, np.uint8, 255)
    ts = [vs.Transform.of(*rng.uniform(-0.03, 0.03, 2), *rng.uniform(-2.5, 2.5, 2)) for _ in range(n)]
    want = R.batch(vs, src, ts, w, h, roi, 16, 255)
    got = vs.sharpen_batch(src, ts, w, h, 1, 2)
    assert got.shape == (n, 9, 12, 3) and np.array_equal(got, want)
    if n == 70:
        assert min(int((a != b).sum()) for a, b in zip(want, src)) > 0


@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_device_memory_unaligned_frames_and_overlap(gpu_vs, fmt):
    """device memory, enqueue only: dense windows on dwords, and windows that start one element into their buffer with an odd pitch; the guard
    elements around and between the destination's rows stay as they were; a destination that overlaps the source is refused"""
    import torch
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(9 + bits)
    rw, rh, rx, ry = 132, 21, 3, 1
    w, h = rx + rw + 5, ry + rh + 2
    ts = _maps(vs, w, h)
    n = len(ts)
    src = _noise(rng, n, rh, rw, dtype, maxv)
    want = R.batch(vs, src, ts, w, h, (rx, ry, rw, rh), 16, maxv)
    guard = 0x5A if esz == 1 else 0x5A5A
    for off, ss in ((0, 3 * rw), (1, 3 * rw + 7)):
        host = np.zeros(n * rh * ss + 8, dtype)
        host[off:off + n * rh * ss].reshape(n, rh, ss)[:, :, :3 * rw] = src.reshape(n, rh, 3 * rw)
        as_t = lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda()
        dsrc = as_t(host)
        ddst = as_t(np.full(n * rh * ss + 8, guard, dtype))
        torch.cuda.synchronize()
        vs.sharpen_batch_device(dsrc.data_ptr() + off * esz, rh * ss, n, w, h, code, ts, rx, ry, rw, rh, ss, ddst.data_ptr() + off * esz, rh * ss, ss)
        torch.cuda.synchronize()
        got = ddst.cpu().numpy().view(dtype)
        body = got[off:off + n * rh * ss].reshape(n, rh, ss)
        assert np.array_equal(body[:, :, :3 * rw].reshape(n, rh, rw, 3), want), (off, ss)
        assert (body[:, :, 3 * rw:] == guard).all() and (got[:off] == guard).all() and (got[off + n * rh * ss:] == guard).all()
        # in place, and a destination that begins inside the source's last row
        for dst_ptr in (dsrc.data_ptr() + off * esz, dsrc.data_ptr() + (off + (n * rh - 1) * ss) * esz):
            with pytest.raises(vs.VsError, match="error -1"):
                vs.sharpen_batch_device(dsrc.data_ptr() + off * esz, rh * ss, n, w, h, code, ts, rx, ry, rw, rh, ss, dst_ptr, rh * ss, ss)


def test_host_overlap_is_refused(gpu_vs):
    import ctypes
    vs = gpu_vs
    buf = np.zeros((4, 6, 8, 3), np.uint8)
    t2 = (vs.Transform * 2)(vs.Transform.of(), vs.Transform.of())
    p = buf.ctypes.data_as(ctypes.c_void_p)
    fs = 6 * 8 * 3
    call = lambda dst: vs.lib().vs_bgr_sharpen_batch(p, fs, 2, 8, 6, vs.FMT_BGR8, t2, None, 0, 0, 8, 6, 24, ctypes.c_void_p(dst), fs, 24, vs.MEM_HOST, None)
    assert call(p.value) == -1 and call(p.value + fs) == -1 and call(p.value + 2 * fs - 1) == -1
    assert call(p.value + 2 * fs) == 0                                   # side by side is fine
