"""The YCbCr rule's numpy restatement (tests/_ycbcr_ref.py) against a plain per-pixel loop written from the rule's text (include/vs_amd.h:
vs_ycbcr_to_bgr_batch), on 7 x 5 frames of every layout, and the rule's consequences (a) and (b).  No device, no library."""
import numpy as np
import pytest

import _ycbcr_ref as R

W, H, N = 7, 5, 2


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def _loop_to_bgr(y, cb, cr, sub, bits):
    sh, maxv = bits - 8, (1 << bits) - 1
    n, h, w = y.shape
    out = np.zeros((n, h, w, 3), y.dtype)
    for f in range(n):
        for v in range(h):
            for u in range(w):
                c = int(y[f, v, u]) - (16 << sh)
                d = e = 0
                if cb is not None:
                    d = int(cb[f, v >> sub[1], u >> sub[0]]) - (128 << sh)
                    e = int(cr[f, v >> sub[1], u >> sub[0]]) - (128 << sh)
                out[f, v, u, 2] = _clamp((298 * c + 409 * e + 128) >> 8, 0, maxv)
                out[f, v, u, 1] = _clamp((298 * c - 100 * d - 208 * e + 128) >> 8, 0, maxv)
                out[f, v, u, 0] = _clamp((298 * c + 516 * d + 128) >> 8, 0, maxv)
    return out


def _loop_pixel(b, g, r, bits):
    sh, maxv = bits - 8, (1 << bits) - 1
    b, g, r = min(int(b), maxv), min(int(g), maxv), min(int(r), maxv)
    return (_clamp(((66 * r + 129 * g + 25 * b + 128) >> 8) + (16 << sh), 0, maxv),
            _clamp(((-38 * r - 74 * g + 112 * b + 128) >> 8) + (128 << sh), 0, maxv),
            _clamp(((112 * r - 94 * g - 18 * b + 128) >> 8) + (128 << sh), 0, maxv))


def _loop_to_ycbcr(bgr, sub, bits, mono):
    n, h, w, _ = bgr.shape
    bx, by = 1 << sub[0], 1 << sub[1]
    cw, ch = (w + sub[0]) >> sub[0], (h + sub[1]) >> sub[1]
    y = np.zeros((n, h, w), bgr.dtype)
    cb, cr = np.zeros((n, ch, cw), bgr.dtype), np.zeros((n, ch, cw), bgr.dtype)
    for f in range(n):
        for v in range(h):
            for u in range(w):
                y[f, v, u] = _loop_pixel(*bgr[f, v, u], bits)[0]
        for cy in range(ch):
            for cx in range(cw):
                su = sv = cnt = 0
                for dy in range(by):
                    for dx in range(bx):
                        _, a, b = _loop_pixel(*bgr[f, min(cy * by + dy, h - 1), min(cx * bx + dx, w - 1)], bits)
                        su, sv, cnt = su + a, sv + b, cnt + 1
                cb[f, cy, cx] = (su + cnt // 2) // cnt
                cr[f, cy, cx] = (sv + cnt // 2) // cnt
    return (y, None, None) if mono else (y, cb, cr)


@pytest.mark.parametrize("layout", sorted(R.LAYOUTS))
@pytest.mark.parametrize("fmt", sorted(R.FORMATS))
def test_the_restatement_agrees_with_a_per_pixel_loop(fmt, layout):
    _, dtype, bits = R.FORMATS[fmt]
    sub, _, mono = R.LAYOUTS[layout]
    rng = np.random.default_rng(bits * 7 + len(layout))
    top = np.iinfo(dtype).max + 1                       # the whole container range: the clamps fire, BGR samples above maxv occur
    cw, ch = R.chroma_shape(W, H, sub)
    y = rng.integers(0, top, (N, H, W)).astype(dtype)
    y[0, 0, :2] = (0, top - 1)                          # (both clamps fire whatever the draw)
    cb =None if mono else rng.integers(0, top, (N, ch, cw)).astype(dtype)
    cr = None if mono else rng.integers(0, top, (N, ch, cw)).astype(dtype)
    want = _loop_to_bgr(y, cb, cr, sub, bits)
    assert np.array_equal(R.to_bgr(y, cb, cr, sub, bits), want)
    maxv = (1 << bits) - 1
    assert (want == 0).any() and (want == maxv).any()
    bgr = rng.integers(0, top, (N, H, W, 3)).astype(dtype)
    got, ref = R.to_ycbcr(bgr, sub, bits, mono), _loop_to_ycbcr(bgr, sub, bits, mono)
    for g, r in zip(got, ref):
        assert (g is None and r is None) or (g.dtype == dtype and np.array_equal(g, r))


@pytest.mark.parametrize("fmt", sorted(R.FORMATS))
def test_gray_bgr_gives_neutral_chroma_exactly(fmt):
    """(a): b == g == r -> Cb == Cr == 128 << sh, at every level of the container and in every subsampling"""
    _, dtype, bits = R.FORMATS[fmt]
    levels = np.unique(np.concatenate([np.arange(0, np.iinfo(dtype).max + 1, 257 if bits > 8 else 1), [(1 << bits) - 1, np.iinfo(dtype).max]]))
    gray = np.repeat(levels.astype(dtype).reshape(1, 1, -1, 1), 3, axis=3)
    gray = np.repeat(gray, 3, axis=1)
    for sub in ((1, 1), (1, 0), (0, 0)):
        _, cb, cr = R.to_ycbcr(gray, sub, bits)
        assert (cb == 128 << (bits - 8)).all() and (cr == 128 << (bits - 8)).all()


@pytest.mark.parametrize("fmt", sorted(R.FORMATS))
def test_luma_only_gives_gray_bgr(fmt):
    """(b): with no chroma planes b == g == r, for every container value of Y"""
    _, dtype, bits = R.FORMATS[fmt]
    y = np.arange(np.iinfo(dtype).max + 1, dtype=np.int64).astype(dtype).reshape(1, 1, -1)
    out = R.to_bgr(y, None, None, (0, 0), bits)
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 1], out[..., 2])
    assert out.min() == 0 and out.max() == (1 << bits) - 1
