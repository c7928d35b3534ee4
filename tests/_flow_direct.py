"""The dense-flow specification (header comment of vs_flow.hip) a second time, in float64 and in the DIRECT form.

Written from that text, sharing no code with tests/_flow_ref.py and none of its shortcuts: the polynomial expansion is a 2-D
weighted least-squares fit of {1, x, y, x^2, y^2, xy} whose 6 x 6 Gram matrix is built numerically from the 2-D weights and solved by
numpy.linalg (no closed-form inverse-Gram constants, no separable passes); the window is a plain 2-D sum over its offsets; the pyramid
blur is a 2-D Gaussian; every border is np.pad(mode="edge").  tests/test_flow_cpu.py holds _flow_ref.py against this stage by stage:
an error the restatement shares with the kernels (a tap, an offset, a constant) is not shared by this file.
"""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def gauss(sigma, r):
    t = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-t * t / (2.0 * sigma * sigma))
    return g / g.sum()


def neighbourhoods(p, before, after):
    """(h, w, before + after + 1, before + after + 1): the values around every pixel, offsets -before..after, replicated border"""
    return sliding_window_view(np.pad(p, ((before, after), (before, after)), mode="edge"), (before + after + 1, before + after + 1))


def layers(w, h, pyr_scale, levels):
    return [(max(1, int(math.floor(w * pyr_scale ** k + 0.5))), max(1, int(math.floor(h * pyr_scale ** k + 0.5))), pyr_scale ** k)
            for k in range(levels + 1)]


def resample(p, w_out, h_out):
    """bilinear samples of p at ((x + 0.5) * w/w_out - 0.5, (y + 0.5) * h/h_out - 0.5), the coordinate clamped to the plane"""
    h, w = p.shape

    def axis(n_out, n_in):
        s = np.clip((np.arange(n_out) + 0.5) * float(np.float32(n_in / n_out)) - 0.5, 0.0, n_in - 1.0)
        i0 = np.floor(s).astype(int)
        return i0, np.minimum(i0 + 1, n_in - 1), s - i0
    x0, x1, tx = axis(w_out, w)
    y0, y1, ty = axis(h_out, h)
    tx, ty = tx[None, :], ty[:, None]
    return ((p[np.ix_(y0, x0)] * (1 - tx) + p[np.ix_(y0, x1)] * tx) * (1 - ty) + (p[np.ix_(y1, x0)] * (1 - tx) + p[np.ix_(y1, x1)] * tx) * ty)


def pyramid_level(img, w_k, h_k, scale):
    L0 = np.asarray(img, np.float64)
    if scale == 1.0:
        return L0
    sigma = (1.0 / scale - 1.0) / 2.0
    r = max(1, int(math.ceil(3.0 * sigma)))
    g = gauss(sigma, r)
    blurred = np.einsum("hwij,ij->hw", neighbourhoods(L0, r, r), np.outer(g, g))
    return resample(blurred, w_k, h_k)


def poly_exp(L, poly_n, poly_sigma):
    """(5, h, w): b1, b2, a11, a22, a12 of the weighted least-squares fit f(p + (x, y)) ~ c + b1 x + b2 y + a11 x^2 + a22 y^2 + 2 a12 x y"""
    n = poly_n
    g = gauss(poly_sigma, n)
    yy, xx = np.mgrid[-n:n + 1, -n:n + 1].astype(np.float64)
    wt = np.outer(g, g).ravel()                                        # weight of offset (y, x)
    B = np.stack([np.ones_like(xx), xx, yy, xx * xx, yy * yy, xx * yy], axis=-1).reshape(-1, 6)
    gram = B.T @ (wt[:, None] * B)
    fit = np.linalg.solve(gram, B.T * wt[None, :])                     # 6 x K: coefficients = fit @ neighbourhood
    nb = neighbourhoods(np.asarray(L, np.float64), n, n)
    c = np.einsum("ck,hwk->chw", fit, nb.reshape(nb.shape[0], nb.shape[1], -1))
    return np.stack([c[1], c[2], c[3], c[4], 0.5 * c[5]])


def sample(p, fx, fy):
    """bilinear sample of p at (fx, fy), both already inside the plane"""
    h, w = p.shape
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    tx, ty = fx - x0, fy - y0
    return (p[y0, x0] * (1 - tx) + p[y0, x1] * tx) * (1 - ty) + (p[y1, x0] * (1 - tx) + p[y1, x1] * tx) * ty


def update(R0, R1, dx, dy):
    """(5, h, w): the entries G11, G12, G22 of A^T A and h1, h2 of A^T db"""
    h, w = dx.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    fx, fy = np.clip(x + dx, 0.0, w - 1.0), np.clip(y + dy, 0.0, h - 1.0)
    S = [sample(R1[c], fx, fy) for c in range(5)]
    A = np.empty((h, w, 2, 2))
    A[..., 0, 0] = (R0[2] + S[2]) / 2
    A[..., 1, 1] = (R0[3] + S[3]) / 2
    A[..., 0, 1] = A[..., 1, 0] = (R0[4] + S[4]) / 2
    d = np.stack([dx, dy], axis=-1)
    db = np.stack([R0[0] - S[0], R0[1] - S[1]], axis=-1) / 2 + np.einsum("hwij,hwj->hwi", A, d)
    G = np.einsum("hwki,hwkj->hwij", A, A)
    hv = np.einsum("hwki,hwk->hwi", A, db)
    return np.stack([G[..., 0, 0], G[..., 0, 1], G[..., 1, 1], hv[..., 0], hv[..., 1]])


def blur_solve(M, winsize, with_det=False):
    before, after = winsize // 2, winsize - 1 - winsize // 2
    m = [neighbourhoods(np.asarray(M[c], np.float64), before, after).sum(axis=(2, 3)) for c in range(5)]
    det = m[0] * m[2] - m[1] * m[1]
    den = np.maximum(det, 0.0) + 1e-3
    dx, dy = (m[2] * m[3] - m[1] * m[4]) / den, (m[0] * m[4] - m[1] * m[3]) / den
    return (dx, dy, det) if with_det else (dx, dy)


def dense_flow(prev, nxt, pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2):
    """((h, w, 2) flow, the smallest determinant of every layer-0 solve as an (h, w) plane)"""
    h, w = np.asarray(prev).shape
    flow, det_min = None, None
    for k in range(levels, -1, -1):
        wk, hk, s = layers(w, h, pyr_scale, levels)[k]
        R0 = poly_exp(pyramid_level(prev, wk, hk, s), poly_n, poly_sigma)
        R1 = poly_exp(pyramid_level(nxt, wk, hk, s), poly_n, poly_sigma)
        if flow is None:
            dx, dy = np.zeros((hk, wk)), np.zeros((hk, wk))
        else:
            dx, dy = resample(flow[..., 0], wk, hk) / pyr_scale, resample(flow[..., 1], wk, hk) / pyr_scale
        det_min = None
        for it in range(iterations):
            dx, dy, det = blur_solve(update(R0, R1, dx, dy), winsize, with_det=True)
            det_min = det if det_min is None else np.minimum(det_min, det)
        flow = np.stack([dx, dy], axis=-1)
    return flow, det_min
