"""The temporal-denoise rule (include/vs_amd.h: vs_bgr_denoise_batch) in numpy on top of the CPU oracle.

Kernel level: every candidate's samples are the oracle's own WARP_BILINEAR_CV warp of that frame, its coverage is tests/_fill_ref.py's
covered() (all four taps of the warp's integer source position inside the frame); weights, sums and the rounded division are int64 numpy
(every value of the rule fits 32 bits: the header's bound, asserted here).  Engine level: tests/_engine_model.py (the candidate lists: its
lookahead_candidates(); the pass comes behind deblur: its target is the deblurred frame, its candidates stay the input frames).

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np

import _fill_ref as FR


def denoise_target(O, target, cands, bits, max_value, strength=24, want_weight=False):
    """one output frame.  target (h, w, 3); cands: [(frame (h, w, 3), oracle Transform)] in list order.  -> the frame; want_weight: also
    sum_j w_j (h, w) int64"""
    h, w, _ = target.shape
    t = int(strength)
    assert 1 <= t <= 255 and len(cands) <= 15
    s = bits - 8
    p = target.astype(np.int64)
    acc = t * p
    sw = np.zeros((h, w), np.int64)
    for img, tr in cands:
        cov = FR.covered(O, tr, w, h)
        if not cov.any():
            continue
        q = O.bgr_image_warp(img, tr, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=max_value).astype(np.int64)
        d = np.abs(p - q).max(axis=2) >> s
        wt = np.where(cov & (d < t), t - d, 0)
        acc = acc + wt[..., None] * q
        sw = sw + wt
    W = t + sw
    num = 2 * acc + W[..., None]
    assert num.max() < 2 ** 30 and W.max() <= 4080                      # the header's bound
    out = np.where((sw == 0)[..., None], p, np.minimum(num // (2 * W[..., None]), max_value)).astype(target.dtype)
    return (out, sw) if want_weight else out


def denoise_frame(O, src, cand_frame, cand_t, bits, max_value, strength=24, want_weight=False):
    """src (n_src, h, w, 3); cand_frame: indices (a negative one ends the list); cand_t: oracle Transforms (entry 0 is ignored)"""
    assert cand_frame[0] >= 0
    cands = []
    for f, t in zip(cand_frame[1:], cand_t[1:]):
        if int(f) < 0:
            break
        cands.append((src[int(f)], t))
    return denoise_target(O, src[int(cand_frame[0])], cands, bits, max_value, strength, want_weight)


def denoise_batch(O, src, cand_frame, cand_t, bits, max_value, strength=24):
    return np.stack([denoise_frame(O, src, list(cf), list(ct), bits, max_value, strength) for cf, ct in zip(cand_frame, cand_t)])


def noisy_clip(synth, w, h, n, seed, noise, bits=8, margin=128, **path_kw):
    """a synth clip (video_stabilizer_amd.synth: its textures, camera path and sampler) with Gaussian noise of `noise` 8-bit levels on every
    frame -> (frames (n, h, w, 3), the noise-free renders (n, h, w, 3), path)"""
    max_value = (1 << bits) - 1
    dtype = np.uint8 if bits == 8 else np.uint16
    path = synth.camera_path(n, seed, **path_kw)
    texs = [synth.base_texture(w + 2 * margin, h + 2 * margin, seed + c, max_value) for c in range(3)]
    rng = np.random.default_rng(seed + 99)
    frames = np.empty((n, h, w, 3), dtype)
    truth = np.empty((n, h, w, 3), dtype)
    for i, t in enumerate(path):
        for c in range(3):
            v = synth.sample_bilinear(texs[c], t, w, h, margin)
            truth[i, :, :, c] = np.clip(np.floor(v + 0.5), 0, max_value)
            v = v + rng.normal(0, noise * max_value / 255.0, v.shape)
            frames[i, :, :, c] = np.clip(np.floor(v + 0.5), 0, max_value)
    return frames, truth, path
