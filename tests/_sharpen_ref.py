"""THE SHARPEN RULE (include/vs_amd.h: vs_bgr_sharpen_batch; csrc/vs_sharpen.hip) in numpy int64, on tests/_fill_ref.py's cv_round_sat / wrap32
and table terms -- the positions are the fill's, to the letter -- and the premise experiment of DESIGN.md section 28 on the oracle's plain warp.

    positions            X, Y (five fraction bits) of every full-frame pixel for the FORWARD transform t
    eligible             the window's eligible pixels
    sharpen / batch      the rule on one window / on n windows under their own transforms
    sharpen_float        the same rule written directly in float64: floor(num / 32768 + 1/2)
    texture, fourier_shift, psnr, grad_energy, premise_case    the premise: a periodic band-limited texture shifted by a sub-pixel phase

V: a module with cv_inverse_matrix(t, w, h) and Transform -- the oracle or video_stabilizer_amd.capi (host functions only).  Test infrastructure
only: nothing of the product's kernels is used here.
"""
import numpy as np

import _fill_ref as RF

NUM_BOUND = 32 * 512 * 131070                                            # the rule's bound on |num|
assert NUM_BOUND == 2147450880 and NUM_BOUND < 2 ** 31 - 16384


def positions(V, t, w, h):
    """(X, Y): int64 (h, w), the int32 positions with five fraction bits of cv::warpAffine's tables, as the fill has them"""
    X0, Y0, ad, bd = RF._table_terms(V, t, w, h, RF.cv_round_sat)
    X = RF.wrap32(RF.wrap32(X0 + 16) + ad) >> 5
    Y = RF.wrap32(RF.wrap32(Y0 + 16) + bd) >> 5
    return X, Y


def covered(X, Y, w, h):
    sx, sy = X >> 5, Y >> 5
    return (sx >= 0) & (sx + 1 <= w - 1) & (sy >= 0) & (sy + 1 <= h - 1)


def _window(a, roi):
    x, y, rw, rh = roi
    return a[y:y + rh, x:x + rw]


def eligible(V, t, w, h, roi):
    """(roi_h, roi_w) bool"""
    X, Y = positions(V, t, w, h)
    cov = _window(covered(X, Y, w, h), roi)
    el = np.zeros(cov.shape, bool)
    if cov.shape[0] >= 3 and cov.shape[1] >= 3:
        el[1:-1, 1:-1] = cov[1:-1, 1:-1] & cov[1:-1, :-2] & cov[1:-1, 2:] & cov[:-2, 1:-1] & cov[2:, 1:-1]
    return el


def _terms(V, img, t, w, h, roi):
    """eligibility, the two weights and the two second differences (zero where the pixel is not interior), int64"""
    X, Y = positions(V, t, w, h)
    a, b = _window(X, roi) & 31, _window(Y, roi) & 31
    va, vb = a * (32 - a), b * (32 - b)
    assert va.min() >= 0 and va.max() <= 256 and vb.min() >= 0 and vb.max() <= 256
    c = img.astype(np.int64)
    lx, ly = np.zeros_like(c), np.zeros_like(c)
    if c.shape[0] >= 3 and c.shape[1] >= 3:
        lx[1:-1, 1:-1] = 2 * c[1:-1, 1:-1] - c[1:-1, :-2] - c[1:-1, 2:]
        ly[1:-1, 1:-1] = 2 * c[1:-1, 1:-1] - c[:-2, 1:-1] - c[2:, 1:-1]
    return eligible(V, t, w, h, roi), va[..., None], vb[..., None], c, lx, ly


def numerators(V, img, t, w, h, roi=None, strength=16):
    """num of every sample (0 where the pixel is not eligible), int64"""
    roi = (0, 0, w, h) if roi is None else roi
    assert img.shape[:2] == (roi[3], roi[2])
    el, va, vb, c, lx, ly = _terms(V, img, t, w, h, roi)
    num = strength * (va * lx + vb * ly)
    assert np.abs(num).max(initial=0) <= NUM_BOUND
    return np.where(el[..., None], num, 0)


def sharpen(V, img, t, w, h, roi=None, strength=16, max_value=None):
    """one window img (roi_h, roi_w, 3) of the w x h output frame made under the FORWARD transform t; roi = (x, y, roi_w, roi_h)"""
    if max_value is None:
        max_value = 255 if img.dtype == np.uint8 else 65535
    num = numerators(V, img, t, w, h, roi, strength)
    delta = (num + 16384) >> 15
    c = img.astype(np.int64)
    return np.where(delta != 0, np.clip(c + delta, 0, max_value), c).astype(img.dtype)


def batch(V, src, ts, w, h, roi=None, strength=16, max_value=None):
    src = np.asarray(src)
    if len(src) == 0:
        return src.copy()
    return np.stack([sharpen(V, f, t, w, h, roi, strength, max_value) for f, t in zip(src, ts)])


def sharpen_float(V, img, t, w, h, roi=None, strength=16, max_value=None):
    """the rule in float64: out = c + floor(num / 32768 + 1/2), every product exact in a double (|num| < 2^31)"""
    roi = (0, 0, w, h) if roi is None else roi
    if max_value is None:
        max_value = 255 if img.dtype == np.uint8 else 65535
    el, va, vb, c, lx, ly = _terms(V, img, t, w, h, roi)
    cf = c.astype(np.float64)
    num = float(strength) * (va.astype(np.float64) * lx.astype(np.float64) + vb.astype(np.float64) * ly.astype(np.float64))
    delta = np.floor(num / 32768.0 + 0.5)
    out = np.where(el[..., None] & (delta != 0), np.clip(cf + delta, 0.0, float(max_value)), cf)
    return out.astype(img.dtype)


# ---- the premise ----------------------------------------------------------------------------------------------------
def texture(n, cut, seed=0):
    """n x n periodic float64 texture: uniform noise under a Gaussian low-pass exp(-(f / cut)^2 / 2), f in cycles per pixel, scaled to 20 .. 235"""
    rng = np.random.default_rng(seed)
    f = np.fft.fftfreq(n)
    g = np.exp(-0.5 * (f[:, None] ** 2 + f[None, :] ** 2) / cut ** 2)
    img = np.real(np.fft.ifft2(np.fft.fft2(rng.uniform(0.0, 1.0, (n, n))) * g))
    return 20.0 + (img - img.min()) * (215.0 / (img.max() - img.min()))


def fourier_shift(img, dx, dy):
    """img(x + dx, y + dy) of the periodic float image"""
    n = img.shape[0]
    f = np.fft.fftfreq(n)
    ph = np.exp(2j * np.pi * (f[None, :] * dx + f[:, None] * dy))
    return np.real(np.fft.ifft2(np.fft.fft2(img) * ph))


def psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b) ** 2))


def grad_energy(img):
    """mean squared forward difference of a periodic image"""
    v = img.astype(np.float64)
    return float(np.mean((np.roll(v, -1, 1) - v) ** 2 + (np.roll(v, -1, 0) - v) ** 2))


def premise_case(O, cut, a, b, strengths=(16,), n=256, pad=8):
    """-> {0: (psnr, ge), strength: (psnr, ge), ..} of the texture shifted by (a / 32, b / 32) with the oracle's VS_WARP_BILINEAR_CV (0: the plain
    warp) and then sharpened by the restatement, against the Fourier shift of the un-rounded texture.  The periodic texture is handed to the warp
    with `pad` wrapped pixels a side, and the middle n x n is judged"""
    tex = texture(n, cut)
    wide = np.pad(np.rint(tex), pad, mode="wrap").astype(np.uint8)
    frame = np.repeat(wide[:, :, None], 3, axis=2)
    w = h = n + 2 * pad
    t = O.Transform.of(0.0, 0.0, -a / 32.0, -b / 32.0)                   # output (x, y) samples the source at (x + a / 32, y + b / 32)
    X, Y = positions(O, t, w, h)
    assert ((X & 31) == a).all() and ((Y & 31) == b).all()
    truth = fourier_shift(tex, a / 32.0, b / 32.0)
    warped = O.bgr_image_warp(frame, t, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT)
    mid = lambda f: f[pad:pad + n, pad:pad + n, 0]
    ge0 = grad_energy(truth)
    res = {0: (psnr(mid(warped), truth), grad_energy(mid(warped)) / ge0)}
    for s in strengths:
        out = sharpen(O, warped, t, w, h, strength=s)
        res[s] = (psnr(mid(out), truth), grad_energy(mid(out)) / ge0)
    return res
