"""The temporal-denoise rule (include/vs_amd.h: vs_bgr_denoise_batch) in numpy on top of the CPU oracle, and the engine's model of it.

Kernel level: every candidate's samples are the oracle's own WARP_BILINEAR_CV warp of that frame, its coverage is tests/_fill_ref.py's
covered() (all four taps of the warp's integer source position inside the frame); weights, sums and the rounded division are int64 numpy
(every value of the rule fits 32 bits: the header's bound, asserted here).  Engine level: the CPU oracle's Stabilizer frame by frame
(tests/_deblur_ref.py's measure() and candidates(): chain_j = compose(T_{k+1}, ..., T_j), cand_t = inverse(chain_j)); order deblur, denoise,
warp, fill.

Test infrastructure only: nothing of the product is used here (the deblur stage of the engine model takes the host algebra's
cv_inverse_matrix from its caller, as tests/_deblur_ref.py does).
"""
import numpy as np

import _deblur_ref as DB
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


def engine_model(O, frames, ahead, strength=24, bits=None, max_value=None, mode="right", deblur=0, cvinv=None, fill=0, **params):
    """the oracle's Stabilizer over one clip with every frame denoised before its warp -> {k: output frame k} (cropped like the engine's) and
    {k: the denoised frame k}.  deblur > 0 (cvinv: the host algebra's cv_inverse_matrix): the deblur in front of it, default parameters -- the
    denoise target is the deblurred frame, its candidates stay the input frames.  fill > 0: the border fill behind the warp, its candidate 0
    the denoised frame, its other candidates the input frames."""
    n, h, w, _ = frames.shape
    if bits is None:
        bits = 8 if frames.dtype == np.uint8 else 10
    if max_value is None:
        max_value = (1 << bits) - 1
    meas, succ, due, p = DB.measure(O, frames, **params)
    crop = max(p.crop_pixels, 0)
    sharp = DB.sharpness_batch(frames, bits) if deblur else None
    outs, clean = {}, {}
    for k, (plain, acc) in due.items():
        tgt = frames[k]
        if deblur:
            cf, ct = DB.candidates(O, k, deblur, meas, succ)
            tgt = DB.deblur_frame(cvinv, frames, sharp, cf, ct, bits, max_value)
        cf, ct = DB.candidates(O, k, ahead, meas, succ, mode)
        d = denoise_target(O, tgt, [(frames[f], t) for f, t in zip(cf[1:], ct[1:]) if f >= 0], bits, max_value, strength)
        clean[k] = d
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
            stack = np.concatenate([d[None], frames])       # (frame 0 of the stack: the denoised frame; frame j + 1: input frame j)
            full = FR.fill_frame(O, stack, ff, ft, p.warp_border, max_value)
        else:
            t = Ck if p.warp_mode == O.WARP_BILINEAR_CV else O.t_inverse(Ck)
            full = O.bgr_image_warp(d, t, p.warp_mode, border=p.warp_border, max_value=max_value)
        outs[k] = full[crop:h - crop, crop:w - crop] if crop else full
    return outs, clean


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
