"""The inpaint rule (include/vs_amd.h: vs_bgr_fill_coverage_batch, vs_bgr_inpaint_batch) in vectorised numpy: the coverage index on top of
tests/_fill_ref.py's covered(), and the push-pull as whole-array operations in int64.

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np

import _fill_ref as F


def coverage_frame(O, cand_frame, cand_t, w, h, roi=None):
    """(h, w) uint8 of one output frame: 1 + the first candidate that covers the pixel, 0 for none; a negative index ends the list"""
    cov = np.zeros((h, w), np.uint8)
    for c, (f, t) in enumerate(zip(cand_frame, cand_t)):
        if f < 0:
            break
        take = F.covered(O, t, w, h) & (cov == 0)
        cov[take] = 1 + c
    if roi is not None:
        x, y, rw, rh = roi
        cov = cov[y:y + rh, x:x + rw]
    return cov


def coverage_batch(O, cand_frame, cand_t, w, h, roi=None):
    return np.stack([coverage_frame(O, list(cf), list(ct), w, h, roi) for cf, ct in zip(cand_frame, cand_t)])


def _push(v, m):
    """level l (H, W, 3) int64 with mask (H, W) bool -> level l+1"""
    H, W = m.shape
    H1, W1 = (H + 1) >> 1, (W + 1) >> 1
    vp = np.zeros((2 * H1, 2 * W1, 3), np.int64)
    mp = np.zeros((2 * H1, 2 * W1), bool)
    vp[:H, :W] = np.where(m[..., None], v, 0)             # (values outside the mask are not read: they are replaced before they are summed)
    mp[:H, :W] = m
    n = mp.reshape(H1, 2, W1, 2).sum((1, 3)).astype(np.int64)
    s = vp.reshape(H1, 2, W1, 2, 3).sum((1, 3))
    nn = np.maximum(n, 1)[..., None]
    return np.where(n[..., None] > 0, (2 * s + nn) // (2 * nn), 0), n > 0


def _near_far(n, n1):
    i = np.arange(n)
    p = i >> 1
    return p, np.clip(p + np.where(i & 1, 1, -1), 0, n1 - 1)


def _pull(v, m, up):
    """level l with its undefined pixels taken from the completely defined level l+1"""
    H, W = m.shape
    py, qy = _near_far(H, up.shape[0])
    px, qx = _near_far(W, up.shape[1])
    est = (9 * up[py][:, px] + 3 * up[py][:, qx] + 3 * up[qy][:, px] + up[qy][:, qx] + 8) >> 4
    return np.where(m[..., None], v, est)


def inpaint(img, mask):
    """img (H, W, 3) uint8 / uint16, mask (H, W) non-zero = keep -> the inpainted window, same dtype; img is not changed"""
    m = np.asarray(mask) != 0
    v = np.asarray(img).astype(np.int64)
    levels = [(v, m)]
    while levels[-1][1].shape != (1, 1):
        levels.append(_push(*levels[-1]))
    if not levels[-1][1][0, 0]:
        return np.array(img, copy=True)
    up = levels[-1][0]
    for v_l, m_l in reversed(levels[:-1]):
        up = _pull(v_l, m_l, up)
    return np.where(m[..., None], img, up.astype(img.dtype))


def inpaint_batch(imgs, masks):
    return np.stack([inpaint(i, m) for i, m in zip(imgs, masks)])
