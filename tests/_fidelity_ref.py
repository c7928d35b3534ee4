"""THE FIDELITY RULE (video_stabilizer_amd/csrc/vs_fidelity.hip, include/vs_amd.h) restated in numpy: int64 arrays inside the bounds the rule states
(asserted here), Python integers for the sums over an image, float64 for the one division per window.  numpy's int64 -> float64 conversion, its
float64 division and np.rint are correctly rounded with ties to even, and nothing here can contract into an fma."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

C1, C2 = 26634, 239708
M64 = (1 << 64) - 1
LIMIT = 532924508                                                        # the rule's bound on vars, |cov|, A, |B|, C, D


def clamp(img, bits):
    return np.minimum(np.asarray(img).astype(np.int64), (1 << bits) - 1)


def gray(img, bits):
    """(h, w, 3) samples -> (h, w) int64 gray levels 0 .. 255"""
    v = clamp(img, bits)
    g = (v[..., 0] * 3735 + v[..., 1] * 19235 + v[..., 2] * 9798 + 16384)
    assert int(g.max(initial=0)) < (1 << 32)
    return np.minimum((g >> 15) >> (bits - 8), 255)


def n_windows(w, h):
    nwx = (w - 8) // 4 + 1 if w >= 8 else 0
    nwy = (h - 8) // 4 + 1 if h >= 8 else 0
    return nwx, nwy


def window_sums(ga, gb):
    """the four sums of every window, (nwy, nwx) int64 each: s1, s2, ss, s12"""
    h, w = ga.shape
    nwx, nwy = n_windows(w, h)
    if nwx == 0 or nwy == 0:
        z = np.zeros((0, 0), np.int64)
        return z, z, z, z

    def sw(z):
        s = sliding_window_view(z, (8, 8))[::4, ::4].sum(axis=(2, 3))
        assert s.shape == (nwy, nwx)
        return s
    return sw(ga), sw(gb), sw(ga * ga + gb * gb), sw(ga * gb)


def factors(s1, s2, ss, s12):
    """vars, cov, A, B, C, D of the rule (int64 arrays or Python ints)"""
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    cov = 64 * s12 - s1 * s2
    return vars_, cov, 2 * s1 * s2 + C1, 2 * cov + C2, s1 * s1 + s2 * s2 + C1, vars_ + C2


def window_q(s1, s2, ss, s12):
    """q of every window, int64; the rule's bounds are asserted on the way"""
    s1, s2, ss, s12 = (np.asarray(v, np.int64) for v in (s1, s2, ss, s12))
    vars_, cov, A, B, C, D = factors(s1, s2, ss, s12)
    if s1.size:
        assert int(max(s1.max(), s2.max())) <= 16320 and int(ss.max()) <= 8323200
        for v in (vars_, cov, A, B, C, D):
            assert int(np.abs(v).max()) <= LIMIT
        assert int(vars_.min()) >= 0 and int(C.min()) >= C1 and int(D.min()) >= C2
        assert int(np.abs(A * B).max()) < (1 << 59) and int((C * D).max()) < (1 << 59)
    q = np.rint(((A * B).astype(np.float64) / (C * D).astype(np.float64)) * 65536.0).astype(np.int64)
    assert q.size == 0 or int(np.abs(q).max()) <= 65536
    return q


def pair_stats(a, b, bits):
    """the six words of one pair as Python integers (ssim_sum in two's complement)"""
    va, vb = clamp(a, bits), clamp(b, bits)
    assert va.shape == vb.shape and va.ndim == 3 and va.shape[2] == 3
    d = va - vb
    sse = [int((d[..., c] * d[..., c]).sum(dtype=np.int64)) for c in range(3)]          # < 65535^2 * 2^30 < 2^62
    ga, gb = gray(a, bits), gray(b, bits)
    sse_y = int(((ga - gb) ** 2).sum(dtype=np.int64))
    q = window_q(*window_sums(ga, gb))
    nwx, nwy = n_windows(va.shape[1], va.shape[0])
    assert q.size == nwx * nwy
    return sse + [sse_y, nwx * nwy, sum(int(v) for v in q.ravel()) & M64]


def stats_batch(a, b, pairs, bits):
    """(n_pairs, 6) uint64; a pair named twice is computed once"""
    out = np.zeros((len(pairs), 6), np.uint64)
    seen = {}
    for i, (ia, ib) in enumerate(pairs):
        key = (int(ia), int(ib))
        if key not in seen:
            seen[key] = np.array(pair_stats(a[key[0]], b[key[1]], bits), dtype=np.uint64)
        out[i] = seen[key]
    return out


def ssim_sum_signed(word):
    word = int(word)
    return word - (1 << 64) if word >> 63 else word


def scores(words, w, h, bits):
    """psnr_b, psnr_g, psnr_r, psnr, psnr_y, ssim of one pair's six words, with Python's math.log10"""
    peak, n = float((1 << bits) - 1), float(w) * float(h)

    def psnr(p2n, sse):
        return math.inf if sse == 0 else 10.0 * math.log10(p2n / float(sse))
    sb, sg, sr, sy, nw, sm = (int(v) for v in words)
    return [psnr(peak * peak * n, sb), psnr(peak * peak * n, sg), psnr(peak * peak * n, sr), psnr(peak * peak * (3.0 * n), sb + sg + sr),
            psnr(255.0 * 255.0 * n, sy), math.nan if nw == 0 else float(ssim_sum_signed(sm)) / (65536.0 * nw)]


def clip_means(frames_a, frames_b, bits):
    """what vs_eval_fidelity prints: the means over the pairs (frames_a[i], frames_b[i]) of min(psnr, 100), min(psnr_y, 100) and ssim"""
    h, w = frames_a.shape[1:3]
    rows = [scores(pair_stats(x, y, bits), w, h, bits) for x, y in zip(frames_a, frames_b)]
    return (sum(min(r[3], 100.0) for r in rows) / len(rows), sum(min(r[4], 100.0) for r in rows) / len(rows), sum(r[5] for r in rows) / len(rows))


def itf(frames, bits, inset=0):
    """inter-frame fidelity of a clip: consecutive frames, the image being the frame minus `inset` pixels on every side"""
    f = frames[:, inset:frames.shape[1] - inset, inset:frames.shape[2] - inset]
    return clip_means(f[:-1], f[1:], bits)
