"""The deblur rule written directly from its specification, in float64 throughout: no fp32, no operation order borrowed from the kernels, no call
into the library (tests/_deblur_ref.py restates the kernels' order and takes its maps from vs_cv_inverse_matrix; a mistake shared by the two --
operand order, which gray is subtracted, which side of the division the ratio sits on -- shows against this form).

Per pixel of target frame k, with the candidates j that take part (S_j > S_k):

    out = (p + sum_j w_j q_j) / (1 + sum_j w_j)         w_j = r_j^2 / (|g_k - g_j| + sensitivity),  r_j = min(S_j / max(S_k, 1), max_ratio)

q_j: candidate j's sample nearest to the position the target pixel maps to under the inverse of the candidate's centre-based similarity
(the centre vs_cv_inverse_matrix documents: ((w - 1) / 2, (h - 1) / 2)), inverted here as a 3 x 3 matrix.  The gray is the rule's integer gray.

THE fp32 ERROR BOUND used when this form is compared with the restatement or the kernel (u = 2^-24, all terms non-negative, so no
cancellation): r_j carries one rounding (the cast), r_j^2 two more and the product's own (3 u), d + sensitivity one, the division one (w_j: 5 u),
w_j q_j one more (6 u); the sum of at most 16 terms (p and 15 products) adds one rounding per addition (15 u), likewise W (5 u + 15 u); the
quotient one, the addition of 0.5 one: (6 + 15) + (5 + 15) + 1 + 1 = 43 u relative to the quotient.  BOUND = 48 u (quotient + 1) leaves the
second-order terms room.  Where round(direct) differs from the fp32 result, the float64 quotient lies within BOUND of a .5 boundary, and
the two differ by 1 LSB."""
import numpy as np

U = 2.0 ** -24


def bound(quot):
    return 48 * U * (np.abs(quot) + 1.0)


def gray(img, bits):
    v = img.astype(object)                                           # Python integers
    g = (v[..., 0] * 3735 + v[..., 1] * 19235 + v[..., 2] * 9798 + 16384) // 32768 // (1 << (bits - 8))
    return np.minimum(g.astype(np.int64), 255).astype(np.float64)


def inverse_map(t, w, h):
    """target pixel -> candidate position: the inverse of x' = c + T + R (x - c), R = [[1 + A, -B], [B, 1 + A]], c = ((w - 1) / 2, (h - 1) / 2)"""
    A, B, TX, TY = (float(v) for v in t.tup())
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    F = np.array([[1 + A, -B, cx + TX - (1 + A) * cx + B * cy],
                  [B, 1 + A, cy + TY - B * cx - (1 + A) * cy],
                  [0.0, 0.0, 1.0]])
    return np.linalg.inv(F)


def deblur_frame(src, sharp, cand_frame, cand_t, bits, sensitivity=2.0, max_ratio=4.0):
    """-> the float64 quotient (h, w, 3), unrounded"""
    _, h, w, _ = src.shape
    k = int(cand_frame[0])
    sk = int(sharp[k])
    p = src[k].astype(np.float64)
    gk = gray(src[k], bits)
    num, den = p.copy(), np.ones((h, w))
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    for f, t in zip(cand_frame[1:], cand_t[1:]):
        f = int(f)
        if f < 0:
            break
        sj = int(sharp[f])
        if not sj > sk:
            continue
        r = min(sj / max(sk, 1), float(np.float32(max_ratio)))
        Minv = inverse_map(t, w, h)
        qx = np.rint(Minv[0, 0] * xs + Minv[0, 1] * ys + Minv[0, 2])
        qy = np.rint(Minv[1, 0] * xs + Minv[1, 1] * ys + Minv[1, 2])
        inside = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
        ix, iy = np.where(inside, qx, 0).astype(np.int64), np.where(inside, qy, 0).astype(np.int64)
        q = src[f][iy, ix].astype(np.float64)
        wt = np.where(inside, r * r / (np.abs(gk - gray(src[f], bits)[iy, ix]) + float(np.float32(sensitivity))), 0.0)
        num += wt[..., None] * q
        den += wt
    return num / den[..., None]


def compare(quot, got, max_value):
    """(number of differing samples, violations): got against round(quot); a violation is a difference of more than 1 LSB or one away from
    a .5 boundary of the quotient by more than bound()"""
    want = np.clip(np.floor(quot + 0.5), 0, max_value)
    diff = got.astype(np.float64) - want
    differs = diff != 0
    near = np.abs(quot - np.floor(quot) - 0.5) <= bound(quot)
    bad = (np.abs(diff) > 1) | (differs & ~near)
    return int(differs.sum()), int(bad.sum())
