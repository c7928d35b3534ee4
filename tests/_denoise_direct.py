"""The temporal-denoise rule written directly from its specification in float64: no integer accumulators, no rounded division, no code shared
with tests/_denoise_ref.py beyond the samples, which both take from the oracle's WARP_BILINEAR_CV warp (the rule DEFINES q as that warp's
output) and tests/_fill_ref.py's coverage.  A mistake of the restatement in the weights, the shift, the strict comparison, which sum carries
the target's own weight or the rounding shows against this form.

Per pixel of the target with samples p_c, over the candidates j that cover the pixel with samples q_jc:

    d_j = floor(max_c |p_c - q_jc| / 2^(bits - 8));  w_j = max(t - d_j, 0);  out_c = (t p_c + sum_j w_j q_jc) / (t + sum_j w_j)

Every term is an integer below 2^30, so numerator and denominator are exact in float64 and the quotient is the correctly rounded value of an
exact rational.  The rule's min((2 acc + W) / (2 W), max) with floor division is floor(acc / W + 1/2): round half up.  round-half-up of the
float64 quotient can differ from it only where the exact rational lies within one rounding (2^-53 relative, < 1e-11 absolute at 16 bits) of
a .5 boundary; TIE = 1e-9 is the window the comparison allows, and then the two differ by 1 LSB."""
import numpy as np

import _fill_ref as FR

TIE = 1e-9


def denoise_quotient(O, target, cands, bits, max_value, strength):
    """-> (the float64 quotient (h, w, 3), sum_j w_j (h, w) float64)"""
    h, w, _ = target.shape
    t = float(strength)
    p = target.astype(np.float64)
    num = t * p
    sw = np.zeros((h, w))
    for img, tr in cands:
        q = O.bgr_image_warp(img, tr, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=max_value).astype(np.float64)
        d = np.floor(np.abs(p - q).max(axis=2) / float(1 << (bits - 8)))
        wt = np.where(FR.covered(O, tr, w, h), np.maximum(t - d, 0.0), 0.0)
        num += wt[..., None] * q
        sw += wt
    return num / (t + sw)[..., None], sw


def compare(quot, sw, target, got, max_value):
    """(number of differing samples, violations): got against round-half-up of the quotient (the target itself where no candidate took part);
    a violation is a difference of more than 1 LSB or one where the quotient is further than TIE from a .5 boundary"""
    want = np.where((sw == 0)[..., None], target.astype(np.float64), np.minimum(np.floor(quot + 0.5), max_value))
    diff = got.astype(np.float64) - want
    differs = diff != 0
    near = np.abs(quot - np.floor(quot) - 0.5) <= TIE
    bad = (np.abs(diff) > 1) | (differs & ~near)
    return int(differs.sum()), int(bad.sum())
