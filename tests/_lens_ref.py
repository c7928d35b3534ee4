"""The radial lens map's rule (include/vs_amd.h: vs_lens_map) and the remap's sample rule (vs_bgr_remap_batch) in numpy.

The map: float64 numpy, one ufunc per rounded operation, in the order the rule writes them; cv_round_sat from tests/_fill_ref.py.  The remap:
VS_WARP_BILINEAR_CV's two blends as tests/_rolling_ref.py restates them (8-bit containers: int64; 16-bit containers: float32 ufuncs, one per
rounded operation), with the clamp border and the constant border.  Then the direction test's renders: an analytic scene seen through the
forward lens model.

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np

import _fill_ref as FR

F32 = np.float32
FIELDS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "zoom")
BORDER_CLAMP, BORDER_CONSTANT = 0, 1


def params(w, h, **kw):
    """vs_lens_params_default as a dict of float64, fields overridden by keyword"""
    p = dict.fromkeys(FIELDS, 0.0)
    p.update(fx=float(max(w, h)), fy=float(max(w, h)), cx=(w - 1) / 2.0, cy=(h - 1) / 2.0, zoom=1.0)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return {k: np.float64(v) for k, v in p.items()}


def coeffs(c):
    """OpenCV's distCoeffs order -> keywords"""
    return dict(zip(("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"), c))


def lens_map(p, w, h):
    """(h, w, 2) int64: (X, Y) with 5 fraction bits, the rule operation for operation"""
    one, two = np.float64(1.0), np.float64(2.0)
    u = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1))
    v = np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    with np.errstate(all="ignore"):
        x = (u - p["cx"]) / (p["fx"] * p["zoom"])
        y = (v - p["cy"]) / (p["fy"] * p["zoom"])
        r2 = x * x + y * y
        kr = (one + ((p["k3"] * r2 + p["k2"]) * r2 + p["k1"]) * r2) / (one + ((p["k6"] * r2 + p["k5"]) * r2 + p["k4"]) * r2)
        xy2 = two * (x * y)
        xd = x * kr + (p["p1"] * xy2 + p["p2"] * (r2 + two * (x * x)))
        yd = y * kr + (p["p1"] * (r2 + two * (y * y)) + p["p2"] * xy2)
        X = FR.cv_round_sat((p["fx"] * xd + p["cx"]) * np.float64(32.0))
        Y = FR.cv_round_sat((p["fy"] * yd + p["cy"]) * np.float64(32.0))
    return np.stack([X, Y], axis=2)


def taps_inside(pos, w, h):
    """(oh, ow) bool: all four taps of the position lie in the w x h frame"""
    sx, sy = pos[..., 0].astype(np.int64) >> 5, pos[..., 1].astype(np.int64) >> 5
    return (sx >= 0) & (sx + 1 <= w - 1) & (sy >= 0) & (sy + 1 <= h - 1)


def remap(frame, pos, border, max_value):
    """one frame (h, w, 3) through pos (oh, ow, 2) -> (oh, ow, 3): taps at (X >> 5, Y >> 5) and right / below, fractions X & 31, Y & 31"""
    h, w, _ = frame.shape
    X, Y = pos[..., 0].astype(np.int64), pos[..., 1].astype(np.int64)
    sx, sy = X >> 5, Y >> 5
    a1, b1 = (X & 31)[..., None], (Y & 31)[..., None]
    a0, b0 = 32 - a1, 32 - b1
    c0, c1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    taps = [frame[y0, c0], frame[y0, c1], frame[y1, c0], frame[y1, c1]]
    if border == BORDER_CONSTANT:                                    # a tap outside the frame counts as 0, weights unchanged
        ins = [(c0 == sx) & (y0 == sy), (c1 == sx + 1) & (y0 == sy), (c0 == sx) & (y1 == sy + 1), (c1 == sx + 1) & (y1 == sy + 1)]
        taps = [np.where(m[..., None], t, 0).astype(frame.dtype) for t, m in zip(taps, ins)]
    else:
        assert border == BORDER_CLAMP
    wts = (a0 * b0, a1 * b0, a0 * b1, a1 * b1)
    if frame.dtype == np.uint8:
        s = sum(t.astype(np.int64) * wt for t, wt in zip(taps, wts)) + 512
        return (s >> 10).astype(np.uint8)
    k = F32(1.0) / F32(1024.0)
    fw = [(p.astype(F32) * k).astype(F32) for p in wts]
    s = (taps[0].astype(F32) * fw[0]).astype(F32)
    for t, wt in zip(taps[1:], fw[1:]):
        s = (s + (t.astype(F32) * wt).astype(F32)).astype(F32)
    return np.clip(np.rint(s).astype(np.int64), 0, max_value).astype(frame.dtype)


def remap_batch(src, pos, border, max_value):
    return np.stack([remap(f, pos, border, max_value) for f in src])


# ---- the direction test's renders ---------------------------------------------------------------------------------------------------------
DIRECTION_COEFFS = [(-0.25, 0.05, 0.001, -0.002), (0.2, 0, 0, 0), (-0.3, 0.1, 0.0005, 0.0005, -0.01, 0.01)]


def distort(p, x, y):
    """the forward model in plain float64 on normalised coordinates: where the ideal point (x, y) lands"""
    r2 = x * x + y * y
    kr = (1 + ((p["k3"] * r2 + p["k2"]) * r2 + p["k1"]) * r2) / (1 + ((p["k6"] * r2 + p["k5"]) * r2 + p["k4"]) * r2)
    return (x * kr + p["p1"] * 2 * x * y + p["p2"] * (r2 + 2 * x * x), y * kr + p["p1"] * (r2 + 2 * y * y) + p["p2"] * 2 * x * y)


def undistort(p, xd, yd, steps=30):
    """its inverse by `steps` fixed-point steps (x <- (xd - tangential(x)) / kr(x))"""
    x, y = xd.copy(), yd.copy()
    for _ in range(steps):
        r2 = x * x + y * y
        kr = (1 + ((p["k3"] * r2 + p["k2"]) * r2 + p["k1"]) * r2) / (1 + ((p["k6"] * r2 + p["k5"]) * r2 + p["k4"]) * r2)
        dx = p["p1"] * 2 * x * y + p["p2"] * (r2 + 2 * x * x)
        dy = p["p1"] * (r2 + 2 * y * y) + p["p2"] * 2 * x * y
        x, y = (xd - dx) / kr, (yd - dy) / kr
    return x, y


def scene(seed):
    """six sinusoids with periods of 12 .. 40 px in random directions: a function of pixel coordinates, values in 128 +- 120"""
    rng = np.random.default_rng(seed)
    period, ang, ph = rng.uniform(12, 40, 6), rng.uniform(0, np.pi, 6), rng.uniform(0, 2 * np.pi, 6)
    return lambda px, py: 128.0 + 20.0 * sum(np.sin(2 * np.pi * (np.cos(a) * px + np.sin(a) * py) / t + f) for t, a, f in zip(period, ang, ph))


def lens_renders(p, w, h, seed):
    """-> (the frame an ideal camera with p's fx, fy, cx, cy sees, the frame the lens p delivers), 8-bit BGR"""
    S = scene(seed)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    to8 = lambda a: np.repeat(np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)[..., None], 3, axis=2)
    x, y = undistort(p, (u - p["cx"]) / p["fx"], (v - p["cy"]) / p["fy"])        # raw pixel (u, v) shows the ideal camera's point (x, y)
    xd, yd = distort(p, x, y)
    assert np.abs(xd * p["fx"] + p["cx"] - u).max() < 1e-6 and np.abs(yd * p["fy"] + p["cy"] - v).max() < 1e-6      # the inversion converged
    return to8(S(u, v)), to8(S(x * p["fx"] + p["cx"], y * p["fy"] + p["cy"]))


def direction_errors(correct, w=160, h=120, seeds=(1, 2, 3)):
    """[(raw, corrected, corrected with the coefficients negated)]: mean absolute error against the ideal camera's frame over the pixels whose
    position (all four taps, under the true coefficients) lies inside the frame.  correct(frame (h, w, 3) uint8, params dict) -> the corrected
    frame"""
    out = []
    for c in DIRECTION_COEFFS:
        p = params(w, h, fx=120.0, fy=120.0, **coeffs(c))
        neg = params(w, h, fx=120.0, fy=120.0, **coeffs([-k for k in c]))
        inside = taps_inside(lens_map(p, w, h), w, h)
        assert inside.mean() > 0.5
        for seed in seeds:
            ideal, raw = lens_renders(p, w, h, seed)
            err = lambda a: float(np.abs(a.astype(np.float64) - ideal)[inside].mean())
            out.append((err(raw), err(correct(raw, p)), err(correct(raw, neg))))
    return out
