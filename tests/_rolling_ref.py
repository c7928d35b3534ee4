"""The rolling-shutter rule (include/vs_amd.h: vs_bgr_rolling_batch) in numpy.

Kernel level: the row time, the row matrix and the int32 position are float64 / int64 numpy, one ufunc per rounded operation, in the order the
rule writes them, on the helpers of tests/_fill_ref.py (cv_round_sat, wrap32); the two blends of VS_WARP_BILINEAR_CV are restated here (8-bit
containers: int64; 16-bit containers: float32 ufuncs, one per rounded operation).  Engine level: tests/_engine_model.py (the motion is
candidate 1 of its lookahead_candidates(); the pass is the last before the warp).

Test infrastructure only: nothing of the product is used here (cvinv, the host algebra's cv_inverse_matrix, comes from the caller, as in
tests/_deblur_ref.py).
"""
import numpy as np

import _fill_ref as FR

F32 = np.float32


def row_times(h, rho):
    """tau(y) = rho * ((double)(2 y - (h - 1)) / (double)(2 h))"""
    ys = np.arange(h, dtype=np.int64)
    return np.float64(rho) * ((2 * ys - (h - 1)).astype(np.float64) / np.float64(2 * h))


def row_matrices(M, h, rho):
    """(h, 6): r0 = 1 + tau (M0 - 1), r1 = tau M1, r2 = tau M2, r3 = tau M3, r4 = 1 + tau (M4 - 1), r5 = tau M5"""
    M = np.asarray(M, np.float64).reshape(6)
    tau = row_times(h, rho)
    with np.errstate(all="ignore"):
        return np.stack([1.0 + tau * (M[0] - 1.0), tau * M[1], tau * M[2], tau * M[3], 1.0 + tau * (M[4] - 1.0), tau * M[5]], axis=1)


def positions(M, w, h, rho):
    """(X, Y), each (h, w) int64 with 5 fraction bits: cv_pos(cv_row_origin(r1, r2, y), cv_row_origin(r4, r5, y), cv_delta(r0, x), cv_delta(r3, x))"""
    r = row_matrices(M, h, rho)
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)
    with np.errstate(all="ignore"):
        X0 = FR.wrap32(FR.cv_round_sat((r[:, 1] * ys + r[:, 2]) * 1024.0) + 16)[:, None]
        Y0 = FR.wrap32(FR.cv_round_sat((r[:, 4] * ys + r[:, 5]) * 1024.0) + 16)[:, None]
        ad = FR.cv_round_sat(r[:, 0][:, None] * xs * 1024.0)
        bd = FR.cv_round_sat(r[:, 3][:, None] * xs * 1024.0)
    return FR.wrap32(X0 + ad) >> 5, FR.wrap32(Y0 + bd) >> 5


def blend(frame, X, Y, max_value):
    """VS_WARP_BILINEAR_CV's blend of the four taps at (X >> 5, Y >> 5), fractions X & 31, Y & 31, columns and rows clamped into the frame"""
    h, w, _ = frame.shape
    sx, sy = X >> 5, Y >> 5
    a1, b1 = (X & 31)[..., None], (Y & 31)[..., None]
    a0, b0 = 32 - a1, 32 - b1
    c0, c1 = np.clip(sx, 0, w - 1), np.clip(sx + 1, 0, w - 1)
    y0, y1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    v00, v01, v10, v11 = frame[y0, c0], frame[y0, c1], frame[y1, c0], frame[y1, c1]
    if frame.dtype == np.uint8:
        i = np.int64
        s = v00.astype(i) * (a0 * b0) + v01.astype(i) * (a1 * b0) + v10.astype(i) * (a0 * b1) + v11.astype(i) * (a1 * b1) + 512
        return (s >> 10).astype(np.uint8)
    k = F32(1.0) / F32(1024.0)
    w00, w01, w10, w11 = [(p.astype(F32) * k).astype(F32) for p in (a0 * b0, a1 * b0, a0 * b1, a1 * b1)]
    s = (v00.astype(F32) * w00).astype(F32)
    for v, wt in ((v01, w01), (v10, w10), (v11, w11)):
        s = (s + (v.astype(F32) * wt).astype(F32)).astype(F32)
    return np.clip(np.rint(s).astype(np.int64), 0, max_value).astype(frame.dtype)


def rolling_frame(frame, M, rho, max_value):
    """one output frame.  M: vs_cv_inverse_matrix of the motion to the following frame (6 doubles), or None: no motion known"""
    if M is None:
        return frame.copy()
    h, w, _ = frame.shape
    X, Y = positions(M, w, h, rho)
    return blend(frame, X, Y, max_value)


def rolling_batch(cvinv, src, cand_frame, cand_t, rho, max_value):
    """src (n_src, h, w, 3); cand_frame (n_out, 2); cand_t: n_out rows of 2 transforms of cvinv's module"""
    _, h, w, _ = src.shape
    return np.stack([rolling_frame(src[int(cf[0])], cvinv(ct[1], w, h) if int(cf[1]) >= 0 else None, rho, max_value)
                     for cf, ct in zip(cand_frame, cand_t)])


def model_positions(M, w, h, rho):
    """the model in plain float64, no fixed point: where the scene point that a global shutter shows at (x, y) sits in the raw frame,
    p + tau(y) (M p - p) -> (px, py) in pixels"""
    M = np.asarray(M, np.float64).reshape(6)
    tau = row_times(h, rho)[:, None]
    xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    mx, my = M[0] * xs + M[1] * ys + M[2], M[3] * xs + M[4] * ys + M[5]
    return xs + tau * (mx - xs), ys + tau * (my - ys)


# ---- the direction test's renders ---------------------------------------------------------------------------------------------------------
def binomial_noise(rng, w, h, margin=24):
    """uniform noise blurred by a 1-4-6-4-1 binomial both ways, float64, (h + 2 margin, w + 2 margin)"""
    a = rng.uniform(0, 255, (h + 2 * margin + 4, w + 2 * margin + 4))
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    a = sum(k[i] * a[i:i + h + 2 * margin] for i in range(5))
    return sum(k[i] * a[:, i:i + w + 2 * margin] for i in range(5))


def bilinear(tex, px, py):
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    fx, fy = px - x0, py - y0
    x0, y0 = np.clip(x0, 0, tex.shape[1] - 2), np.clip(y0, 0, tex.shape[0] - 2)
    return (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy


def shutter_renders(tex, w, h, motion, rho, margin=24):
    """a camera that moves by `motion` = (dx, dy, angle) per frame period, uniformly, about the frame's centre; time 0 is the middle row's.
    -> (the global-shutter frame at time 0, the rolling-shutter frame with row y exposed at tau(y), the forward transform (A, B, TX, TY) of
    the motion to the following frame in VS_WARP_BILINEAR_CV's convention: frame(t = 0) = warp(frame(t = 1), that)), 8-bit BGR"""
    dx, dy, ang = motion
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))

    def render(t):                                                   # frame pixel p at time t shows texture point c + R(t a)(p - c) + t d
        c, s = np.cos(t * ang), np.sin(t * ang)
        px = cx + c * (xs - cx) - s * (ys - cy) + t * dx
        py = cy + s * (xs - cx) + c * (ys - cy) + t * dy
        return bilinear(tex, px + margin, py + margin)
    tau = row_times(h, rho)[:, None] * np.ones((1, w))
    to8 = lambda v: np.repeat(np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)[..., None], 3, axis=2)
    # the following frame (time 1) shows at pixel q what this frame (time 0) shows at p = c + R(a)(q - c) + d.  The forward transform that
    # warps the following frame onto this one sends q to p: that is the candidate transform, and its inverse matrix M sends p to q
    return to8(render(0.0)), to8(render(tau)), (np.cos(ang) - 1.0, np.sin(ang), dx, dy)
