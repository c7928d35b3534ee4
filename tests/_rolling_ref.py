"""The rolling-shutter rule (include/vs_amd.h: vs_bgr_rolling_batch) in numpy, and the engine's model of it.

Kernel level: the row time, the row matrix and the int32 position are float64 / int64 numpy, one ufunc per rounded operation, in the order the
rule writes them, on the helpers of tests/_fill_ref.py (cv_round_sat, wrap32); the two blends of VS_WARP_BILINEAR_CV are restated here (8-bit
containers: int64; 16-bit containers: float32 ufuncs, one per rounded operation).  Engine level: the CPU oracle's Stabilizer frame by frame
(tests/_deblur_ref.py's measure() and candidates()); order deblur, denoise, rolling shutter, warp, fill.

Test infrastructure only: nothing of the product is used here (cvinv, the host algebra's cv_inverse_matrix, comes from the caller, as in
tests/_deblur_ref.py).
"""
import numpy as np

import _deblur_ref as DB
import _denoise_ref as DN
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


def engine_model(O, frames, rho, cvinv=None, bits=None, max_value=None, deblur=0, denoise=0, fill=0, inpaint=None, **params):
    """the oracle's Stabilizer over one clip with every frame corrected before its warp -> {k: output frame k} (cropped like the engine's) and
    {k: the corrected frame k}.  Order: deblur (cvinv: the host algebra's cv_inverse_matrix; default parameters), denoise (default strength),
    rolling shutter (the motion: candidate 1 of the look-ahead list, inverse(T_{k+1}); a failed alignment or lag 0: none), warp, fill (its
    candidate 0 the corrected frame, its other candidates the input frames), inpaint (with the fill only: tests/_inpaint_ref.py's
    inpaint(window, keep mask) on what the fill leaves open in the output window)."""
    n, h, w, _ = frames.shape
    if bits is None:
        bits = 8 if frames.dtype == np.uint8 else 10
    if max_value is None:
        max_value = (1 << bits) - 1
    if cvinv is None:
        cvinv = O.cv_inverse_matrix
    meas, succ, due, p = DB.measure(O, frames, **params)
    crop = max(p.crop_pixels, 0)
    sharp = DB.sharpness_batch(frames, bits) if deblur else None
    outs, fixed = {}, {}
    for k, (plain, acc) in due.items():
        tgt = frames[k]
        if deblur:
            cf, ct = DB.candidates(O, k, deblur, meas, succ)
            tgt = DB.deblur_frame(cvinv, frames, sharp, cf, ct, bits, max_value)
        if denoise:
            cf, ct = DB.candidates(O, k, denoise, meas, succ)
            tgt = DN.denoise_target(O, tgt, [(frames[f], t) for f, t in zip(cf[1:], ct[1:]) if f >= 0], bits, max_value)
        cf, ct = DB.candidates(O, k, min(1, p.lag), meas, succ)
        M = cvinv(ct[1], w, h) if len(cf) > 1 and cf[1] >= 0 else None
        d = rolling_frame(tgt, M, rho, max_value) if rho != 0 else tgt
        fixed[k] = d
        Ck = O.t_inverse(acc)
        if fill > 0:
            ff, ft = [0], [Ck]
            chain = O.Transform.of()
            for j in range(k + 1, k + fill + 1):
                if not succ[j]:
                    break
                chain = O.t_compose(chain, meas[j])
                ff.append(j + 1)
                ft.append(O.t_compose(O.t_inverse(chain), Ck))
            stack = np.concatenate([d[None], frames])       # (frame 0 of the stack: the corrected frame; frame j + 1: input frame j)
            full, _, still_open = FR.fill_frame(O, stack, ff, ft, p.warp_border, max_value, want_masks=True)
            if inpaint is not None:                         # (the window is the cropped frame: the push-pull sees nothing outside it)
                full = full.copy()
                win = (slice(crop, h - crop), slice(crop, w - crop))
                full[win] = inpaint(full[win], ~still_open[win])
        else:
            t = Ck if p.warp_mode == O.WARP_BILINEAR_CV else O.t_inverse(Ck)
            full = O.bgr_image_warp(d, t, p.warp_mode, border=p.warp_border, max_value=max_value)
        outs[k] = full[crop:h - crop, crop:w - crop] if crop else full
    return outs, fixed


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
