"""Hostile inputs for the sharpen pass (include/vs_amd.h: vs_bgr_sharpen_batch): the maps of tests/_hostile_maps.py (NaN, infinite, singular,
near-singular, saturating), column terms on cvRound ties, samples above the format's maximum, all-0 beside all-maximum columns, and windows that
lie inside poison on four sides with guard words around the destination.  Against the restatement (tests/_sharpen_ref.py) bit for bit; every
builder asserts its premise on the restatement before anything is handed to the kernel."""
import numpy as np
import pytest

import _fill_ref as RF
import _hostile_maps as H
import _sharpen_ref as R

pytestmark = pytest.mark.gpu

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr16": (4, np.uint16, 16)}
SHAPES = [((5, 3), (0, 0)), ((64, 9), (1, 3)), ((67, 10), (0, 0)), ((260, 9), (3, 1))]


def _noise(rng, n, h, w, dtype, maxv):
    return rng.integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_hostile_maps(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(600 + bits)
    names = sorted(H.HOSTILE) + sorted(H.FILL_EXTREME)
    maps = [H.HOSTILE.get(k) or H.FILL_EXTREME[k] for k in names]
    changed = 0
    for (rw, rh), (rx, ry) in SHAPES:
        w, h = rx + rw + (rx and 3), ry + rh + (ry and 2)
        ts = [vs.Transform.of(*m) for m in maps]
        src = _noise(rng, len(ts), rh, rw, dtype, maxv)
        with np.errstate(all="ignore"):
            want = R.batch(vs, src, ts, w, h, (rx, ry, rw, rh), 32, maxv)
        all_nan = 0
        for k, name in enumerate(names):
            with np.errstate(all="ignore"):
                M = np.asarray(vs.cv_inverse_matrix(ts[k], w, h), np.float64)
            if np.isnan(M).all() or not M.any():                         # premise: a matrix of NaNs, or of zeros, leaves every pixel on phase 0
                assert np.array_equal(want[k], src[k]), name
                all_nan += 1
        assert all_nan == 3                                              # nan_A, nan_B, singular
        changed += int((want != src).sum())
        got = vs.sharpen_batch(src, ts, w, h, rx, ry, params=vs.sharpen_params(strength=32), fmt=code)
        bad = [names[k] for k in range(len(ts)) if not np.array_equal(got[k], want[k])]
        assert not bad, (rw, rh, rx, ry, bad)
    assert changed > 1000                                                # some of the extreme maps do sharpen (quarter turns, zooms)


def _half_up_positions(V, t, w, h):
    """the positions with cvRound replaced by floor(v + 1/2): NOT the rule"""
    rnd = lambda v: np.floor(np.asarray(v, np.float64) + 0.5).astype(np.int64)
    X0, Y0, ad, bd = RF._table_terms(V, t, w, h, rnd)
    return RF.wrap32(RF.wrap32(X0 + 16) + ad) >> 5, RF.wrap32(RF.wrap32(Y0 + 16) + bd) >> 5


def test_cvround_ties(gpu_vs):
    """a zoom of 2048 / 2049 makes M0 = M4 = 2049 / 2048 exactly: cvRound(M0 x 1024) = cvRound(1024 x + x / 2) is a tie at every odd x, and likewise
    the row origins at every odd y.  Ties go to even: rounding half up instead moves some positions by 1 / 1024 across a 1 / 32 step and changes
    the output there"""
    vs = gpu_vs
    w, h = 200, 70
    rng = np.random.default_rng(11)
    src, ts = [], []
    differ = 0
    for tx, ty in ((0.0, 0.0), (-15.0 / 1024, 0.25), (0.5 / 1024, -1.5 / 1024), (3.0 + 17.0 / 1024, 1.0 / 64)):
        t = vs.Transform.of(2048.0 / 2049.0 - 1.0, 0.0, tx, ty)
        M = np.asarray(vs.cv_inverse_matrix(t, w, h), np.float64)
        assert M[0] == 2049.0 / 2048.0 and M[4] == M[0] and M[1] == 0 and M[3] == 0
        v = M[0] * np.arange(w, dtype=np.float64) * 1024
        assert ((v - np.floor(v)) == 0.5).sum() == w // 2
        X, Y = R.positions(vs, t, w, h)
        Xh, Yh = _half_up_positions(vs, t, w, h)
        differ += int(((X != Xh) | (Y != Yh)).sum())
        ts.append(t)
        src.append(_noise(rng, 1, h, w, np.uint8, 255)[0])
    assert differ > 100                                                  # premise: the ties decide positions
    src = np.stack(src)
    want = R.batch(vs, src, ts, w, h, None, 16, 255)
    assert (want != src).mean() > 0.3
    assert np.array_equal(vs.sharpen_batch(src, ts, w, h), want)


def test_samples_above_the_maximum_and_both_clamps(gpu_vs):
    """10-bit containers holding 65535 here and there; all-0 beside all-maximum columns at strength 32, where c + delta leaves the range both ways"""
    vs = gpu_vs
    T = vs.Transform.of
    rng = np.random.default_rng(5)
    w, h = 70, 20
    ts = [T(0, 0, 0.5, 0.5), T(0, 0, -0.5, 0), T(0.03, 0.05, 1.25, -0.75)]
    src = _noise(rng, len(ts), h, w, np.uint16, 1023)
    src[rng.random(src.shape[:3]) < 0.1] = 65535
    want = R.batch(vs, src, ts, w, h, None, 16, 1023)
    assert ((want == src) & (src > 1023)).any() and ((want != src) & (src > 1023)).any()
    assert np.array_equal(vs.sharpen_batch(src, ts, w, h, fmt=2), want)
    for dtype, maxv, code in ((np.uint8, 255, 1), (np.uint16, 65535, 4)):
        bars = np.zeros((len(ts), h, w, 3), dtype)
        bars[:, :, ::2] = maxv
        want = R.batch(vs, bars, ts, w, h, None, 32, maxv)
        num = R.numerators(vs, bars[0], ts[0], w, h, strength=32)
        c = bars[0].astype(np.int64)
        assert (c + ((num + 16384) >> 15) > maxv).any() and (c + ((num + 16384) >> 15) < 0).any()      # premise: both clamps are live
        if maxv == 65535:
            assert np.abs(num).max() == R.NUM_BOUND // 2                 # (one axis of the bound's two, at its largest)
        assert np.array_equal(vs.sharpen_batch(bars, ts, w, h, params=vs.sharpen_params(strength=32), fmt=code), want)


@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_windows_inside_poison_with_guard_words(gpu_vs, fmt):
    """device memory: every window lies in a larger surface whose other elements are poison -- the extreme value beside noise, so a tap outside the
    window would change the result -- and the destination windows lie in a surface of guard words that must stay as they were"""
    import torch
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(40 + bits)
    T = vs.Transform.of
    guard = 0x5A if esz == 1 else 0x5A5A
    as_t = lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda()
    # (columns in front, columns behind, rows above and below every window); the second keeps every row on a dword, the others do not
    for (rw, rh), (left, right, top, bot) in (((67, 10), (1, 2, 2, 3)), ((256, 9), (4, 8, 1, 2)), ((4, 3), (3, 3, 1, 1))):
        w, h = rw + 9, rh + 6
        ts = [T(0, 0, 0.5, 0.5), T(0.03, 0.05, 1.25, -0.75), T(-0.25, 0.12, 0.4, -0.3), T(0, 0, -0.25, 0.75)]
        n = len(ts)
        src = _noise(rng, n, rh, rw, dtype, maxv)
        want = R.batch(vs, src, ts, w, h, (2, 3, rw, rh), 32, maxv)
        assert (want != src).any()
        ss, fh = 3 * (left + rw + right), top + rh + bot
        surf = np.full((n, fh, ss), maxv, dtype)                         # poison: the largest second difference against any sample
        surf[:, top:top + rh, 3 * left:3 * (left + rw)] = src.reshape(n, rh, 3 * rw)
        dsrc = as_t(surf.reshape(-1))
        ddst = as_t(np.full(n * fh * ss, guard, dtype))
        first = (top * ss + 3 * left) * esz
        torch.cuda.synchronize()
        vs.sharpen_batch_device(dsrc.data_ptr() + first, fh * ss, n, w, h, code, ts, 2, 3, rw, rh, ss, ddst.data_ptr() + first, fh * ss, ss,
                                params=vs.sharpen_params(strength=32))
        torch.cuda.synchronize()
        got = ddst.cpu().numpy().view(dtype).reshape(n, fh, ss)
        assert np.array_equal(got[:, top:top + rh, 3 * left:3 * (left + rw)].reshape(n, rh, rw, 3), want), (rw, rh)
        got[:, top:top + rh, 3 * left:3 * (left + rw)] = guard
        assert (got == guard).all(), (rw, rh)
        assert np.array_equal(dsrc.cpu().numpy().view(dtype).reshape(n, fh, ss), surf)      # the source is only read
