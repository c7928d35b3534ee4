"""CPU restatement of this build's dense optical flow (vs_flow.hip; include/vs_amd.h "Dense optical flow").

numpy float32, in the kernels' exact operation order: every product and every sum is one IEEE rounding, no fused
multiply-add, every sum runs over its taps in ascending offset order from 0.0f.  The kernels are pinned to this file
bit for bit (tests/test_flow_gpu.py).  The specification it restates is two-frame polynomial-expansion flow
(Farneback 2003) with OpenCV's parameter meanings; the arithmetic and the border rules are this build's own and are
listed in the header comment of vs_flow.hip.

Host constants (Gaussian weights, the inverse-G factors of the polynomial fit, level sizes and ratios) are computed in
double exactly as the library computes them and then rounded to float32 once.
"""
import math

import numpy as np

F = np.float32
DEFAULT = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)
REG = F(1e-3)          # added to the (non-negative part of the) determinant of the 2x2 solve


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


# ---- host constants ------------------------------------------------------------------------------------------------
def gauss_double(sigma, r):
    """normalised Gaussian weights for offsets -r..r, in double"""
    e = [math.exp(-float(t * t) / (2.0 * sigma * sigma)) for t in range(-r, r + 1)]
    s = 0.0
    for v in e:
        s += v
    return [v / s for v in e]


def level_geometry(w, h, pyr_scale, levels):
    """[(w_k, h_k, scale_k)] for k = 0..levels (levels + 1 layers; scale_k = pyr_scale multiplied k times)"""
    out = []
    s = 1.0
    for k in range(levels + 1):
        if k:
            s *= pyr_scale
        out.append((max(1, int(math.floor(w * s + 0.5))), max(1, int(math.floor(h * s + 0.5))), s))
    return out


def pyr_taps(scale):
    """blur applied to level 0 before it is resampled to a level of this scale: sigma = (1/scale - 1) / 2"""
    sigma = (1.0 / scale - 1.0) * 0.5
    r = max(1, int(math.ceil(3.0 * sigma)))
    return np.array(gauss_double(sigma, r), F), r


def poly_consts(poly_n, poly_sigma):
    """(g, g*t, g*t^2) for t = -poly_n..poly_n and the inverse-G factors (ig11, ig03, ig33, ig34, ig55), float32"""
    gd = gauss_double(poly_sigma, poly_n)
    ts = range(-poly_n, poly_n + 1)
    g = np.array(gd, F)
    gt = np.array([gd[i] * float(t) for i, t in enumerate(ts)], F)
    gtt = np.array([gd[i] * float(t * t) for i, t in enumerate(ts)], F)
    S0 = S2 = S4 = 0.0
    for i, t in enumerate(ts):
        S0 += gd[i]
        S2 += gd[i] * float(t * t)
        S4 += gd[i] * float(t * t * t * t)
    a, b, c, d = S0 * S0, S0 * S2, S0 * S4, S2 * S2
    D1 = a * (c + d) - 2.0 * b * b
    ig11 = 1.0 / (S2 * S0)
    ig03 = -b / D1
    ig33 = 0.5 * (a / D1 + 1.0 / (c - d))
    ig34 = 0.5 * (a / D1 - 1.0 / (c - d))
    ig55 = 0.5 / (S2 * S2)
    return g, gt, gtt, tuple(F(v) for v in (ig11, ig03, ig33, ig34, ig55))


# ---- stages --------------------------------------------------------------------------------------------------------
def _vsum(p, taps, lo):
    """sum_t taps[t] * p[clamp(y + lo + t)], ascending t (taps None: plain box sum of len(lo..))"""
    h = p.shape[0]
    acc = np.zeros(p.shape, F)
    for i, wt in enumerate(taps):
        rows = np.clip(np.arange(h) + lo + i, 0, h - 1)
        acc = acc + (p[rows] if wt is None else F(wt) * p[rows])
    return acc


def _hsum(p, taps, lo):
    w = p.shape[1]
    acc = np.zeros(p.shape, F)
    for i, wt in enumerate(taps):
        cols = np.clip(np.arange(w) + lo + i, 0, w - 1)
        acc = acc + (p[:, cols] if wt is None else F(wt) * p[:, cols])
    return acc


def _coords(n_out, n_in, ratio):
    """source coordinate of output sample i under the centre-aligned map ((i + 0.5) * ratio - 0.5), clamped: (i0, i1, t)"""
    s = (np.arange(n_out, dtype=F) + F(0.5)) * F(ratio) - F(0.5)
    s = np.fmin(np.fmax(s, F(0.0)), F(n_in - 1))
    i0 = s.astype(np.int32)
    return i0, np.minimum(i0 + 1, n_in - 1), s - i0.astype(F)


def _bilinear(p, x0, x1, tx, y0, y1, ty):
    """(p[y0,x0]*(1-tx) + p[y0,x1]*tx)*(1-ty) + (p[y1,x0]*(1-tx) + p[y1,x1]*tx)*ty, element-wise on matching index arrays"""
    u, v = F(1.0) - tx, F(1.0) - ty
    top = p[y0, x0] * u + p[y0, x1] * tx
    bot = p[y1, x0] * u + p[y1, x1] * tx
    return top * v + bot * ty


def pyramid_level(img, w_k, h_k, scale):
    """level of a u8 image: level 0 as float; else Gaussian blur (vertical, then horizontal) of level 0 sampled bilinearly"""
    L0 = np.asarray(img, np.uint8).astype(F)
    if scale == 1.0:
        return L0
    h, w = L0.shape
    g, r = pyr_taps(scale)
    H = _hsum(_vsum(L0, g, -r), g, -r)
    x0, x1, tx = _coords(w_k, w, F(w / w_k))
    y0, y1, ty = _coords(h_k, h, F(h / h_k))
    Y0, X0 = np.meshgrid(y0, x0, indexing="ij")
    Y1, X1 = np.meshgrid(y1, x1, indexing="ij")
    TY, TX = np.meshgrid(ty, tx, indexing="ij")
    return _bilinear(H, X0, X1, TX, Y0, Y1, TY)


def poly_exp(L, poly_n, poly_sigma):
    """(5, h, w): b1, b2, a11, a22, a12 -- the local fit f(p + (x, y)) ~ c + b1 x + b2 y + a11 x^2 + a22 y^2 + 2 a12 x y"""
    g, gt, gtt, (ig11, ig03, ig33, ig34, ig55) = poly_consts(poly_n, poly_sigma)
    lo = -poly_n
    v0, v1, v2 = _vsum(L, g, lo), _vsum(L, gt, lo), _vsum(L, gtt, lo)
    h0, hx, hxx = _hsum(v0, g, lo), _hsum(v0, gt, lo), _hsum(v0, gtt, lo)
    hy, hyy, hxy = _hsum(v1, g, lo), _hsum(v2, g, lo), _hsum(v1, gt, lo)
    return np.stack([hx * ig11, hy * ig11, (h0 * ig03 + hxx * ig33) + hyy * ig34, (h0 * ig03 + hyy * ig33) + hxx * ig34,
                     hxy * ig55])


def update(R0, R1, dx, dy):
    """the 5 unique entries of A^T A | A^T db at every pixel for the flow estimate (dx, dy)"""
    h, w = dx.shape
    fx = np.fmin(np.fmax(np.arange(w, dtype=F)[None, :] + dx, F(0.0)), F(w - 1))
    fy = np.fmin(np.fmax(np.arange(h, dtype=F)[:, None] + dy, F(0.0)), F(h - 1))
    x0, y0 = fx.astype(np.int32), fy.astype(np.int32)
    tx, ty = fx - x0.astype(F), fy - y0.astype(F)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = [_bilinear(R1[c], x0, x1, tx, y0, y1, ty) for c in range(5)]
    half = F(0.5)
    a11 = (R0[2] + s[2]) * half
    a22 = (R0[3] + s[3]) * half
    a12 = (R0[4] + s[4]) * half
    bx = (R0[0] - s[0]) * half + (a11 * dx + a12 * dy)
    by = (R0[1] - s[1]) * half + (a12 * dx + a22 * dy)
    return np.stack([a11 * a11 + a12 * a12, a11 * a12 + a12 * a22, a12 * a12 + a22 * a22, a11 * bx + a12 * by,
                     a12 * bx + a22 * by])


def upsample_flow(Fc, w_k, h_k, inv_scale):
    """coarser level's flow (hc, wc, 2) resampled to w_k x h_k and scaled by 1/pyr_scale"""
    hc, wc = Fc.shape[:2]
    x0, x1, tx = _coords(w_k, wc, F(wc / w_k))
    y0, y1, ty = _coords(h_k, hc, F(hc / h_k))
    Y0, X0 = np.meshgrid(y0, x0, indexing="ij")
    Y1, X1 = np.meshgrid(y1, x1, indexing="ij")
    TY, TX = np.meshgrid(ty, tx, indexing="ij")
    return (_bilinear(Fc[..., 0], X0, X1, TX, Y0, Y1, TY) * F(inv_scale),
            _bilinear(Fc[..., 1], X0, X1, TX, Y0, Y1, TY) * F(inv_scale))


def blur_solve(M, winsize):
    """box sum of winsize x winsize (vertical, then horizontal) of the 5 planes, then the regularised 2x2 solve"""
    lo = -(winsize // 2)
    box = [None] * winsize
    m = [_hsum(_vsum(M[c], box, lo), box, lo) for c in range(5)]
    det = m[0] * m[2] - m[1] * m[1]
    idet = F(1.0) / (np.fmax(det, F(0.0)) + REG)
    return (m[2] * m[3] - m[1] * m[4]) * idet, (m[0] * m[4] - m[1] * m[3]) * idet


# ---- the whole flow ------------------------------------------------------------------------------------------------
def check_params(p):
    assert p["flags"] == 0 and 0.0 < p["pyr_scale"] < 1.0 and 0 <= p["levels"] <= 15
    assert 1 <= p["winsize"] <= 31 and 1 <= p["iterations"] and 1 <= p["poly_n"] <= 7 and p["poly_sigma"] > 0


def dense_flow(prev, nxt, **kw):
    """(h, w, 2) float32 flow (dx, dy): prev(x) ~ next(x + d)"""
    p = params(**kw)
    check_params(p)
    prev, nxt = np.asarray(prev, np.uint8), np.asarray(nxt, np.uint8)
    h, w = prev.shape
    geo = level_geometry(w, h, p["pyr_scale"], p["levels"])
    inv = F(1.0 / p["pyr_scale"])
    flow = None
    for k in range(p["levels"], -1, -1):
        wk, hk, s = geo[k]
        R0 = poly_exp(pyramid_level(prev, wk, hk, s), p["poly_n"], p["poly_sigma"])
        R1 = poly_exp(pyramid_level(nxt, wk, hk, s), p["poly_n"], p["poly_sigma"])
        if flow is None:
            dx = np.zeros((hk, wk), F)
            dy = np.zeros((hk, wk), F)
        else:
            dx, dy = upsample_flow(flow, wk, hk, inv)
        M = update(R0, R1, dx, dy)
        for it in range(p["iterations"]):
            dx, dy = blur_solve(M, p["winsize"])
            if it + 1 < p["iterations"]:
                M = update(R0, R1, dx, dy)
        flow = np.stack([dx, dy], axis=-1)
    return flow


def pair_median(flow):
    """element n/2 of the per-pixel magnitudes: selected on dx*dx + dy*dy (float32), then one correctly rounded sqrt"""
    m2 = (flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1]).ravel()
    n = m2.size
    return F(np.sqrt(np.partition(m2, n // 2)[n // 2]))


def median_of_pairs(values):
    """eval_jitter.cpp's median: the middle element, the mean of the two middle ones for an even count (double)"""
    v = sorted(float(x) for x in values)
    if not v:
        return 0.0
    n = len(v) // 2
    return v[n] if len(v) % 2 else 0.5 * (v[n] + v[n - 1])


def gray(frame, bits=8):
    """vs_bgr_to_gray's rule, shifted to 8 bits: (B*3735 + G*19235 + R*9798 + 16384) >> 15 >> (bits - 8), saturated"""
    f = np.asarray(frame).astype(np.uint32)
    g = (f[..., 0] * 3735 + f[..., 1] * 19235 + f[..., 2] * 9798 + 16384) >> 15
    return np.minimum(g >> (bits - 8), 255).astype(np.uint8)


def flow_jitter(frames, bits=8, **kw):
    """(median, pair medians) of a clip of BGR frames (or gray u8 frames when the last axis is not 3)"""
    fr = [gray(f, bits) if f.ndim == 3 else np.asarray(f, np.uint8) for f in frames]
    pm = np.array([pair_median(dense_flow(fr[i], fr[i + 1], **kw)) for i in range(len(fr) - 1)], F)
    return median_of_pairs(pm), pm
