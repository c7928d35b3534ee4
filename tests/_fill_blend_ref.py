"""The fill's blend rule (include/vs_amd.h: vs_bgr_image_warp_fill_blend_batch) in numpy on top of tests/_fill_ref.py and the CPU oracle's
WARP_BILINEAR_CV warp.  Engine level: tests/_engine_model.py (blend=(feather, match) on its fill).

Gains in Python ints (unbounded: the rule's unsigned 64-bit terms stay below 2^63, asserted), everything else in int64.  Candidates, coverage
and positions are _fill_ref's; the plain value p and the sample q of a covering candidate are the oracle's own warp.

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np

import _fill_ref as R


def channel_sums(frames):
    """(n, h, w, 3) -> (n, 3) uint64: the raw samples of every channel summed, no clamp"""
    return np.asarray(frames).astype(np.uint64).sum(axis=(1, 2), dtype=np.uint64)


def gain_q15(sk, sj):
    """the Q15 gain of a candidate whose channel sums to sj for an output frame whose channel sums to sk"""
    sk, sj = int(sk), int(sj)
    if sk == 0 or sj == 0:
        return 32768
    assert 2 * 32768 * sk + sj < 1 << 63
    return min(max((2 * 32768 * sk + sj) // (2 * sj), 16384), 65536)


def matched(q, gains, max_value):
    """f_c = min((q_c G_c + 16384) >> 15, max_value); q (..., 3) integers"""
    g = np.asarray(gains, np.int64)
    v = np.asarray(q, np.int64) * g + 16384
    assert int(v.max(initial=0)) < 1 << 32
    return np.minimum(v >> 15, max_value)


def cv_positions(O, t, w, h):
    """the int32 table positions X, Y (5 fraction bits) of every output pixel, full frame: the rule's, as in _fill_ref.cv_source_ints"""
    X0, Y0, ad, bd = R._table_terms(O, t, w, h, R.cv_round_sat)
    return R.wrap32(R.wrap32(X0 + 16) + ad) >> 5, R.wrap32(R.wrap32(Y0 + 16) + bd) >> 5


def plain_weight(O, t, w, h, feather):
    """(h, w) int64: k = min(d + 1, K) where candidate 0 (forward transform t) covers the pixel, K elsewhere and everywhere with feather == 0"""
    K = 32 << feather
    X, Y = cv_positions(O, t, w, h)
    cov = R._inside(X >> 5, Y >> 5, w, h)
    if feather == 0:
        return np.full((h, w), K, np.int64), cov
    Xmax, Ymax = (w - 1) * 32 - 1, (h - 1) * 32 - 1
    d = np.minimum(np.minimum(X, Xmax - X), np.minimum(Y, Ymax - Y))
    assert (d[cov] >= 0).all()
    return np.where(cov, np.minimum(d + 1, K), K).astype(np.int64), cov


def blend_frame(O, src, cand_frame, cand_t, sums, feather, match, border, max_value=None, roi=None, want_masks=False, plain=None):
    """one output frame.  src (n_src, h, w, 3); cand_frame: indices (a negative one ends the list); cand_t: oracle Transforms; sums (n_src, 3)
    (read with match only).  want_masks: also cov0, still_open (no candidate covers), band (covered, blended with a later candidate).
    plain: the full-frame plain value p, where candidate 0's pixels are not src's (the engine's deblurred / denoised frame)"""
    _, h, w, _ = src.shape
    assert cand_frame[0] >= 0 and 0 <= feather <= 6 and match in (0, 1)
    if max_value is None:
        max_value = 255 if src.dtype == np.uint8 else 65535
    K = 32 << feather
    p = plain if plain is not None else O.bgr_image_warp(src[cand_frame[0]], cand_t[0], O.WARP_BILINEAR_CV, border=border, max_value=max_value)
    assert p.shape == (h, w, 3)
    kk, cov0 = plain_weight(O, cand_t[0], w, h, feather)
    assert np.array_equal(cov0, R.covered(O, cand_t[0], w, h))
    f = np.zeros((h, w, 3), np.int64)
    undecided = np.ones((h, w), bool)               # no later candidate has covered the pixel yet
    wanted = ~cov0 | (kk < K)                        # the pixels whose value may depend on a later candidate
    for j, t in zip(cand_frame[1:], cand_t[1:]):
        if j < 0:
            break
        take = R.covered(O, t, w, h) & undecided & wanted
        if take.any():
            q = O.bgr_image_warp(src[j], t, O.WARP_BILINEAR_CV, border=border, max_value=max_value)[take]
            g = [gain_q15(sums[cand_frame[0]][c], sums[j][c]) if match else 32768 for c in range(3)]
            f[take] = matched(q, g, max_value)
        undecided &= ~take
    has_f = wanted & ~undecided
    out = p.astype(np.int64)
    fillm = ~cov0 & has_f
    out[fillm] = f[fillm]
    band = cov0 & has_f
    kb = kk[band][:, None]
    mix = kb * out[band] + (K - kb) * f[band] + K // 2
    assert int(mix.max(initial=0)) < 1 << 27
    out[band] = mix >> (5 + feather)
    out = out.astype(src.dtype)
    still_open = ~cov0 & ~has_f
    if roi is not None:
        x, y, rw, rh = roi
        out, cov0, still_open, band = (a[y:y + rh, x:x + rw] for a in (out, cov0, still_open, band))
    return (out, cov0, still_open, band) if want_masks else out


def blend_batch(O, src, cand_frame, cand_t, sums, feather, match, border, max_value=None, roi=None):
    return np.stack([blend_frame(O, src, list(cf), list(ct), sums, feather, match, border, max_value, roi) for cf, ct in zip(cand_frame, cand_t)])
