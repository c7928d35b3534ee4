"""The YCbCr <-> BGR rule (include/vs_amd.h: vs_ycbcr_to_bgr_batch, vs_bgr_to_ycbcr_batch) in numpy int64, both directions, every layout.
Written from the rule's text, not from the kernels: BT.601 limited range in 8.8 fixed point, every `>> 8` a floor (numpy's >> on signed
integers is arithmetic), chroma replicated towards BGR, box-averaged over clamped cells towards YCbCr.

Planes: y (n, h, w); cb, cr (n, ch, cw) with ch = (h + sub_y) >> sub_y, cw = (w + sub_x) >> sub_x, or None (luma only).  How the planes lie in
memory (planar, NV12, NV21, pitches) is the caller's business: the rule does not depend on it."""
import numpy as np

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}
# name -> (sub = (sub_x, sub_y), interleaved, mono) as video_stabilizer_amd.capi's host forms take them
LAYOUTS = {"i420": ((1, 1), None, False), "nv12": ((1, 1), "nv12", False), "nv21": ((1, 1), "nv21", False), "i422": ((1, 0), None, False),
           "i444": ((0, 0), None, False), "mono": ((0, 0), None, True)}


def chroma_shape(w, h, sub):
    return (w + sub[0]) >> sub[0], (h + sub[1]) >> sub[1]


def to_bgr(y, cb, cr, sub, bits):
    """-> (n, h, w, 3) of y's dtype"""
    sh, maxv = bits - 8, (1 << bits) - 1
    n, h, w = y.shape
    c = y.astype(np.int64) - (16 << sh)
    if cb is None:
        d = e = np.zeros_like(c)
    else:
        yy, xx = np.arange(h) >> sub[1], np.arange(w) >> sub[0]
        d = cb.astype(np.int64)[:, yy][:, :, xx] - (128 << sh)
        e = cr.astype(np.int64)[:, yy][:, :, xx] - (128 << sh)
    r = np.clip((298 * c + 409 * e + 128) >> 8, 0, maxv)
    g = np.clip((298 * c - 100 * d - 208 * e + 128) >> 8, 0, maxv)
    b = np.clip((298 * c + 516 * d + 128) >> 8, 0, maxv)
    return np.stack([b, g, r], axis=3).astype(y.dtype)


def per_pixel_ycbcr(bgr, bits):
    """the three full-resolution planes, int64"""
    sh, maxv = bits - 8, (1 << bits) - 1
    v = np.minimum(bgr.astype(np.int64), maxv)
    b, g, r = v[..., 0], v[..., 1], v[..., 2]
    y = np.clip(((66 * r + 129 * g + 25 * b + 128) >> 8) + (16 << sh), 0, maxv)
    cb = np.clip(((-38 * r - 74 * g + 112 * b + 128) >> 8) + (128 << sh), 0, maxv)
    cr = np.clip(((112 * r - 94 * g - 18 * b + 128) >> 8) + (128 << sh), 0, maxv)
    return y, cb, cr


def cell_sums(p, sub):
    """(n, h, w) -> the sums over the bx x by cells, the right and bottom edges clamped: pixel (min(cx bx + dx, w - 1), min(cy by + dy, h - 1))"""
    n, h, w = p.shape
    bx, by = 1 << sub[0], 1 << sub[1]
    cw, ch = chroma_shape(w, h, sub)
    xs = np.minimum(np.arange(cw * bx), w - 1)
    ys = np.minimum(np.arange(ch * by), h - 1)
    q = p[:, ys][:, :, xs]
    return q.reshape(n, ch, by, cw, bx).sum(axis=(2, 4))


def to_ycbcr(bgr, sub, bits, mono=False):
    """(n, h, w, 3) -> (y, cb, cr) of bgr's dtype; mono: cb = cr = None"""
    y, cb, cr = per_pixel_ycbcr(bgr, bits)
    if mono:
        return y.astype(bgr.dtype), None, None
    cnt = (1 << sub[0]) * (1 << sub[1])
    avg = (lambda p: ((cell_sums(p, sub) + cnt // 2) // cnt).astype(bgr.dtype))
    return y.astype(bgr.dtype), avg(cb), avg(cr)
