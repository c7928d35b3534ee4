"""The border-fill rule (include/vs_amd.h: vs_bgr_image_warp_fill_batch) in numpy on top of the CPU oracle.

Kernel level: coverage from the oracle's output -> source matrix and cv::warpAffine's table rule (the coding of
tests/test_bilinear_vs_opencv_fixed_point.py), every candidate's pixels from the oracle's own WARP_BILINEAR_CV warp, first covering candidate
wins.  Engine level: tests/_engine_model.py (the candidate lists: its fill_candidates(); the fill takes the place of the plain warp).

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np


INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def cv_round_sat(v):
    """cvRound as the rule has it (vs_device.hpp / the oracle's cv_round_sat): ties to even, saturated to int32, NaN -> 0.  float64 -> int64"""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(v, np.float64))
        r = np.where(np.isnan(r), 0.0, np.clip(r, float(INT32_MIN), float(INT32_MAX)))
    return r.astype(np.int64)


def wrap32(v):
    """an int64 sum taken back into int32 the way two's-complement addition leaves it"""
    return ((np.asarray(v, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _table_terms(O, t, w, h, rnd):
    M = np.asarray(O.cv_inverse_matrix(t, w, h), np.float64).reshape(6)
    xs = np.arange(w, dtype=np.float64)
    ys = np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        ad = rnd(M[0] * xs * 1024)[None, :]
        bd = rnd(M[3] * xs * 1024)[None, :]
        X0 = rnd((M[1] * ys + M[2]) * 1024)
        Y0 = rnd((M[4] * ys + M[5]) * 1024)
    return X0, Y0, ad, bd


def cv_source_ints(O, t, w, h):
    """integer source position (sx, sy) of every output pixel for the FORWARD transform t, full frame: THE RULE -- cvRound saturated to
    int32, + 16 and X0 + adelta wrapping in int32, arithmetic shifts (cv_round_sat, cv_row_origin, cv_pos in vs_device.hpp / vs_fill.hip; the
    oracle's plain warp)"""
    X0, Y0, ad, bd = _table_terms(O, t, w, h, cv_round_sat)
    X = wrap32(wrap32(X0 + 16) + ad) >> 5
    Y = wrap32(wrap32(Y0 + 16) + bd) >> 5
    return X >> 5, Y >> 5


def cv_source_ints_int64(O, t, w, h):
    """the same positions in unbounded (int64) arithmetic: NOT the rule.  Equal to it wherever no term saturates and no sum leaves int32 --
    every moderate transform; kept for the premise assertions of the hostile cases and for tests/test_fill_cpu.py, which pins where the two
    part.  (Non-finite terms have no int64 value: they become 0 here.)"""
    def rnd(v):
        r = np.rint(v)
        return np.where(np.isfinite(r), np.clip(r, -2.0 ** 62, 2.0 ** 62), 0.0).astype(np.int64)
    X0, Y0, ad, bd = _table_terms(O, t, w, h, rnd)
    X = (X0 + 16 + ad) >> 5
    Y = (Y0 + 16 + bd) >> 5
    return X >> 5, Y >> 5


def _inside(sx, sy, w, h):
    return (sx >= 0) & (sx + 1 <= w - 1) & (sy >= 0) & (sy + 1 <= h - 1)


def covered(O, t, w, h):
    """(h, w) bool: all four taps of the pixel lie in the frame"""
    return _inside(*cv_source_ints(O, t, w, h), w, h)


def covered_int64(O, t, w, h):
    """covered() on the int64 positions: premise assertions only"""
    return _inside(*cv_source_ints_int64(O, t, w, h), w, h)


def fill_frame(O, src, cand_frame, cand_t, border, max_value=None, roi=None, want_masks=False):
    """one output frame: src (n_src, h, w, 3); cand_frame: indices (a negative one ends the list); cand_t: oracle Transforms"""
    _, h, w, _ = src.shape
    assert cand_frame[0] >= 0
    out = O.bgr_image_warp(src[cand_frame[0]], cand_t[0], O.WARP_BILINEAR_CV, border=border, max_value=max_value)
    cov0 = covered(O, cand_t[0], w, h)
    open_ = ~cov0
    for f, t in zip(cand_frame[1:], cand_t[1:]):
        if f < 0:
            break
        take = covered(O, t, w, h) & open_
        if take.any():
            out[take] = O.bgr_image_warp(src[f], t, O.WARP_BILINEAR_CV, border=border, max_value=max_value)[take]
        open_ &= ~take
    if roi is not None:
        x, y, rw, rh = roi
        out, cov0, open_ = out[y:y + rh, x:x + rw], cov0[y:y + rh, x:x + rw], open_[y:y + rh, x:x + rw]
    return (out, cov0, open_) if want_masks else out


def fill_batch(O, src, cand_frame, cand_t, border, max_value=None, roi=None):
    return np.stack([fill_frame(O, src, list(cf), list(ct), border, max_value, roi) for cf, ct in zip(cand_frame, cand_t)])
