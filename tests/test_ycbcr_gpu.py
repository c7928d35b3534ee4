"""vs_ycbcr_to_bgr_batch and vs_bgr_to_ycbcr_batch (vs_ycbcr.hip) against the rule's numpy restatement (tests/_ycbcr_ref.py), bit for bit:
every format and layout over shapes chosen for the kernels' seams, dense and on pitched buffers whose padding carries a guard, all 2^24
8-bit triples, more frames than a grid's y extent takes, and the argument errors."""
import ctypes as C

import numpy as np
import pytest

import _ycbcr_ref as R

pytestmark = pytest.mark.gpu

# (1,1), (2,2), (3,3): below a dword; (7,5): odd both ways; (64,8), (65,9): a wave's seam, odd; (256,16), (260,32): the wide form and its
# strip seam; (258,16): refuses the wide form
SHAPES = [(1, 1), (2, 2), (3, 3), (7, 5), (64, 8), (65, 9), (256, 16), (260, 32), (258, 16)]
N = 3


def _noise(rng, shape, dtype):
    """uniform over the whole container: the clamps fire and BGR samples above the format's maximum occur"""
    return rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)


def _planes(rng, n, w, h, sub, mono, dtype):
    cw, ch = R.chroma_shape(w, h, sub)
    y = _noise(rng, (n, h, w), dtype)
    return (y, None, None) if mono else (y, _noise(rng, (n, ch, cw), dtype), _noise(rng, (n, ch, cw), dtype))


def _pitches(w, h, sub, interleaved, mode):
    """(y_stride, c_stride, bgr_stride) in elements: dense, odd (no row but the first starts on a dword) or multiples of 4 elements"""
    cw, _ = R.chroma_shape(w, h, sub)
    crow = cw * (2 if interleaved else 1)
    if mode == "dense":
        return w, crow, 3 * w
    if mode == "odd":
        return (w + 3) | 1, (crow + 5) | 1, (3 * w + 7) | 1
    return (w + 7) & ~3, (crow + 11) & ~3, (3 * w + 9) & ~3


def _takes_wide(w, esz, strides, mono):
    """the wide form's condition on staged buffers (every span starts on a dword there): w % 4 == 0 and every pitch a whole number of dwords"""
    ys, cs, bs = strides
    return w % 4 == 0 and all((s * esz) % 4 == 0 for s in ((ys, bs) if mono else (ys, cs, bs)))


def _own_samples_blanked(bufs, n, w, h, sub, interleaved, guard):
    """the destination buffers of bgr_to_ycbcr_batch with the rows' own samples overwritten by the guard"""
    cw, ch = R.chroma_shape(w, h, sub)
    out = [b.copy() for b in bufs]
    out[0][2:2 + n * h, :w] = guard
    for b in out[1:]:
        b[2:2 + n * ch, :cw * (2 if interleaved else 1)] = guard
    return out


WIDE_SEEN = {"wide": 0, "narrow": 0}


@pytest.mark.parametrize("layout", ["i420", "nv12", "nv21", "i422", "i444", "mono"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10", "bgr12", "bgr16"])
def test_both_directions_equal_the_restatement(gpu_vs, fmt, layout):
    vs = gpu_vs
    code, dtype, bits = R.FORMATS[fmt]
    sub, inter, mono = R.LAYOUTS[layout]
    esz = np.dtype(dtype).itemsize
    guard = 0x5A if esz == 1 else 0x5A5A
    rng = np.random.default_rng(bits * 100 + len(layout) + sub[0] * 7 + sub[1])
    for w, h in SHAPES:
        y, cb, cr = _planes(rng, N, w, h, sub, mono, dtype)
        bgr = _noise(rng, (N, h, w, 3), dtype)
        want_bgr = R.to_bgr(y, cb, cr, sub, bits)
        want_planes = R.to_ycbcr(bgr, sub, bits, mono)
        for mode in ("dense", "odd", "dword"):
            ys, cs, bs = _pitches(w, h, sub, inter, mode)
            WIDE_SEEN["wide" if _takes_wide(w, esz, (ys, cs, bs), mono) else "narrow"] += 1
            got, buf = vs.ycbcr_to_bgr_batch(y, cb, cr, sub=sub, fmt=code, interleaved=inter, y_stride=ys, c_stride=cs, dst_stride=bs, guard=guard)
            assert np.array_equal(got, want_bgr), (w, h, mode, int((got != want_bgr).sum()))
            assert (buf[:, :, 3 * w:] == guard).all(), (w, h, mode)
            planes, bufs = vs.bgr_to_ycbcr_batch(bgr, sub=sub, fmt=code, interleaved=inter, mono=mono, src_stride=bs, y_stride=ys, c_stride=cs, guard=guard)
            for g, r, name in zip(planes, want_planes, "y cb cr".split()):
                assert (g is None and r is None) or np.array_equal(g, r), (w, h, mode, name)
            assert len(bufs) == (1 if mono else 2 if inter else 3)
            assert all((b == guard).all() for b in _own_samples_blanked(bufs, N, w, h, sub, inter, guard)), (w, h, mode)


def test_both_forms_were_exercised():
    """(runs behind the grid above) cases that meet the wide form's condition and cases that do not: more than zero of each kind"""
    assert WIDE_SEEN["wide"] > 0 and WIDE_SEEN["narrow"] > 0, WIDE_SEEN


def _all_triples():
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(1, 4096, 4096)
    return (idx & 255).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), (idx >> 16).astype(np.uint8)


def test_every_8bit_triple_to_bgr(gpu_vs):
    """all 2^24 (Y, Cb, Cr) as one 4096 x 4096 4:4:4 frame"""
    y, cb, cr = _all_triples()
    got = gpu_vs.ycbcr_to_bgr_batch(y, cb, cr, sub=(0, 0))
    for r0 in range(0, 4096, 512):
        s = slice(r0, r0 + 512)
        assert np.array_equal(got[:, s], R.to_bgr(y[:, s], cb[:, s], cr[:, s], (0, 0), 8)), r0


def test_every_8bit_triple_to_ycbcr(gpu_vs):
    """all 2^24 (B, G, R) as one 4096 x 4096 frame, to 4:4:4"""
    bgr = np.stack(_all_triples(), axis=3)
    got = gpu_vs.bgr_to_ycbcr_batch(bgr, sub=(0, 0))
    for r0 in range(0, 4096, 512):
        s = slice(r0, r0 + 512)
        for g, r in zip(got, R.to_ycbcr(bgr[:, s], (0, 0), 8)):
            assert np.array_equal(g[:, s], r), r0


def test_more_frames_than_a_grid_takes(gpu_vs):
    """65 537 frames of 2 x 2 I420: the frames go in gridDim.y, which ends at 65 535"""
    n = 65537
    rng = np.random.default_rng(65537)
    y, cb, cr = _planes(rng, n, 2, 2, (1, 1), False, np.uint8)
    assert np.array_equal(gpu_vs.ycbcr_to_bgr_batch(y, cb, cr), R.to_bgr(y, cb, cr, (1, 1), 8))
    bgr = _noise(rng, (n, 2, 2, 3), np.uint8)
    for g, r in zip(gpu_vs.bgr_to_ycbcr_batch(bgr), R.to_ycbcr(bgr, (1, 1), 8)):
        assert np.array_equal(g, r)
    assert not np.array_equal(bgr[65535], bgr[0]) and not np.array_equal(bgr[65536], bgr[1])       # (the tail is its own frames)


def test_argument_errors_write_nothing(gpu_vs):
    vs = gpu_vs
    w, h, n = 8, 6, 2
    y = np.full((n, h, w), 100, np.uint8)
    c = np.full((n, h // 2, w // 2), 100, np.uint8)
    bgr = np.full((n, h, w, 3), 0x5A, np.uint8)

    def desc(**kw):
        d = vs.ycbcr_planes(y.ctypes.data, c.ctypes.data, c.ctypes.data, w, w // 2, 1, (1, 1), w * h, (w // 2) * (h // 2))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def both(d, ww=w, hh=h, fmt=vs.FMT_BGR8, bs=3 * w, bfs=3 * w * h):
        a = vs.lib().vs_ycbcr_to_bgr_batch(C.byref(d), n, ww, hh, fmt, vs._p(bgr), bfs, bs, vs.MEM_HOST, None)
        b = vs.lib().vs_bgr_to_ycbcr_batch(vs._p(bgr), bfs, n, ww, hh, bs, fmt, C.byref(d), vs.MEM_HOST, None)
        return a, b
    assert both(desc()) == (0, 0)
    y[...] = 100
    c[...] = 100
    bgr[...] = 0x5A
    ARG, UNSUPPORTED = -1, -3
    assert both(desc(c_step=3)) == (ARG, ARG) and both(desc(c_step=0)) == (ARG, ARG)
    assert both(desc(c_step=2, c_stride=w)) == (ARG, ARG)                              # interleaved, but the two pointers are not neighbours
    assert both(desc(sub_x=2)) == (ARG, ARG) and both(desc(sub_y=-1)) == (ARG, ARG)
    assert both(desc(cb=None)) == (ARG, ARG) and both(desc(cr=None)) == (ARG, ARG)
    assert both(desc(y=None)) == (ARG, ARG)
    assert both(desc(y_stride=w - 1)) == (ARG, ARG) and both(desc(c_stride=w // 2 - 1)) == (ARG, ARG)
    assert both(desc(y_frame_stride=w * h - 1)) == (ARG, ARG) and both(desc(c_frame_stride=(w // 2) * (h // 2) - 1)) == (ARG, ARG)
    assert both(desc(), bs=3 * w - 1) == (ARG, ARG) and both(desc(), bfs=3 * w * h - 1) == (ARG, ARG)
    assert both(desc(), fmt=vs.FMT_GRAY8) == (ARG, ARG) and both(desc(), fmt=9) == (ARG, ARG)
    assert both(desc(), ww=0) == (ARG, ARG) and both(desc(), hh=-1) == (ARG, ARG)
    big = desc(y_stride=32768, c_stride=16384, y_frame_stride=1 << 40, c_frame_stride=1 << 40)
    assert both(big, ww=32768, bs=3 * 32768, bfs=1 << 40) == (UNSUPPORTED, UNSUPPORTED)
    assert vs.lib().vs_ycbcr_to_bgr_batch(None, n, w, h, vs.FMT_BGR8, vs._p(bgr), 3 * w * h, 3 * w, vs.MEM_HOST, None) == ARG
    assert vs.lib().vs_ycbcr_to_bgr_batch(C.byref(desc()), n, w, h, vs.FMT_BGR8, None, 3 * w * h, 3 * w, vs.MEM_HOST, None) == ARG
    assert vs.lib().vs_ycbcr_to_bgr_batch(C.byref(desc()), n, w, h, vs.FMT_BGR8, vs._p(bgr), 3 * w * h, 3 * w, 7, None) == ARG      # no such memory
    assert (y == 100).all() and (c == 100).all() and (bgr == 0x5A).all()
