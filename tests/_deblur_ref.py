"""The deblur rule (include/vs_amd.h: vs_bgr_sharpness_batch / vs_bgr_deblur_batch) in numpy, in the kernels' operation order.

Kernel level: int64 sums for the sharpness, float64 maps from cv_inverse_matrix (the host algebra: no device involved), float32 weights
and accumulators with every operation rounded on its own (numpy never fuses a multiply into an add), candidates summed in list order.
Engine level: tests/_engine_model.py (the candidate lists: its lookahead_candidates(); the pass is the first of its chain).

Test infrastructure only: the only product code used is the host algebra (cv_inverse_matrix), handed in by the caller.
"""
import numpy as np

F32 = np.float32


def gray_unclamped(img, bits):
    """the gray before the rule's min(g, 255): above 255 only where a 10- or 12-bit container holds a sample above its format's maximum"""
    v = img.astype(np.int64)
    return ((v[..., 0] * 3735 + v[..., 1] * 19235 + v[..., 2] * 9798 + 16384) >> 15) >> (bits - 8)


def gray8(img, bits):
    """vs_bgr_to_gray's rule shifted to 8 bits: (..., 3) integers -> (...) int64 in 0 .. 255"""
    return np.minimum(gray_unclamped(img, bits), 255)


def sharpness(frame, bits):
    """S of one (h, w, 3) frame, a Python int"""
    g = gray8(frame, bits)
    if g.shape[0] < 3 or g.shape[1] < 3:
        return 0
    dx = g[1:-1, 2:] - g[1:-1, :-2]
    dy = g[2:, 1:-1] - g[:-2, 1:-1]
    return int((dx * dx + dy * dy).sum())


def sharpness_batch(src, bits):
    return np.array([sharpness(f, bits) for f in src], np.uint64)


def sharpness_many(src, bits):
    """sharpness_batch vectorised over the batch (the same integer sums): for batches of many small frames"""
    g = gray8(src, bits)
    if g.shape[1] < 3 or g.shape[2] < 3:
        return np.zeros(len(src), np.uint64)
    dx = g[:, 1:-1, 2:] - g[:, 1:-1, :-2]
    dy = g[:, 2:, 1:-1] - g[:, :-2, 1:-1]
    return (dx * dx + dy * dy).sum(axis=(1, 2)).astype(np.uint64)


def nearest_map(M, w, h):
    """(qx, qy) float64 (h, w): rint((M0 x + M1 y) + M2), rint((M3 x + M4 y) + M5)"""
    M = np.asarray(M, np.float64).reshape(6)
    xs = np.arange(w, dtype=np.float64)[None, :]
    ys = np.arange(h, dtype=np.float64)[:, None]
    return np.rint((M[0] * xs + M[1] * ys) + M[2]), np.rint((M[3] * xs + M[4] * ys) + M[5])


def deblur_frame(cvinv, src, sharp, cand_frame, cand_t, bits, max_value, sensitivity=2.0, max_ratio=4.0, want_weight=False, want_raw=False):
    """one output frame.  src (n_src, h, w, 3); sharp: the S of every frame of src; cand_frame: indices (a negative one ends the list);
    cand_t: Transforms; cvinv(t, w, h) -> the six doubles of vs_cv_inverse_matrix.  want_weight: also W (h, w) float32; want_raw: (out, W,
    floor(acc / W + 0.5) before the saturation, float32 (h, w, 3))"""
    _, h, w, _ = src.shape
    k = int(cand_frame[0])
    assert k >= 0
    sk = int(sharp[k])
    sens = F32(sensitivity)
    part = []
    for f, t in zip(cand_frame[1:], cand_t[1:]):
        f = int(f)
        if f < 0:
            break
        sj = int(sharp[f])
        if sj > sk:
            r = F32(min(float(sj) / float(max(sk, 1)), float(F32(max_ratio))))
            part.append((f, t, F32(r * r)))
    tgt = src[k]
    if not part:
        if want_raw:
            return tgt.copy(), np.ones((h, w), F32), tgt.astype(F32)
        return (tgt.copy(), np.ones((h, w), F32)) if want_weight else tgt.copy()
    gk = gray8(tgt, bits)
    acc = tgt.astype(F32)
    W = np.ones((h, w), F32)
    for f, t, r2 in part:
        qx, qy = nearest_map(cvinv(t, w, h), w, h)
        inside = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)          # (false for NaN)
        ix = np.where(inside, qx, 0).astype(np.int64)
        iy = np.where(inside, qy, 0).astype(np.int64)
        q = src[f][iy, ix]
        d = np.abs(gk - gray8(q, bits)).astype(F32)
        wt = np.where(inside, r2 / (d + sens), F32(0)).astype(F32)
        for c in range(3):
            prod = (wt * q[..., c].astype(F32)).astype(F32)
            acc[..., c] = np.where(inside, acc[..., c] + prod, acc[..., c])
        W = np.where(inside, W + wt, W).astype(F32)
    raw = np.floor((acc / W[..., None]).astype(F32) + F32(0.5))
    out = np.clip(raw, 0, max_value).astype(src.dtype)
    if want_raw:
        return out, W, raw
    return (out, W) if want_weight else out


def deblur_batch(cvinv, src, sharp, cand_frame, cand_t, bits, max_value, sensitivity=2.0, max_ratio=4.0):
    return np.stack([deblur_frame(cvinv, src, sharp, list(cf), list(ct), bits, max_value, sensitivity, max_ratio)
                     for cf, ct in zip(cand_frame, cand_t)])


def blurred_clip(synth, w, h, n, seed, blurred, blur_px=6.0, angle=0.5, noise=1.0, bits=8, margin=128, **path_kw):
    """a synth clip (video_stabilizer_amd.synth: its textures, camera path and sampler) with Gaussian noise of `noise` LSB on every frame and
    the frames listed in `blurred` motion-blurred: the mean of 13 renders along a line of blur_px pixels at `angle`.
    -> (frames (n, h, w, 3), {k: the unblurred, noise-free render of frame k for k in blurred}, path)"""
    max_value = (1 << bits) - 1
    dtype = np.uint8 if bits == 8 else np.uint16
    path = synth.camera_path(n, seed, **path_kw)
    texs = [synth.base_texture(w + 2 * margin, h + 2 * margin, seed + c, max_value) for c in range(3)]
    rng = np.random.default_rng(seed + 99)
    frames = np.empty((n, h, w, 3), dtype)
    truth = {}
    taps = np.linspace(-blur_px / 2, blur_px / 2, 13)
    for i, t in enumerate(path):
        for c in range(3):
            v = synth.sample_bilinear(texs[c], t, w, h, margin)
            if i in blurred:
                truth.setdefault(i, np.empty((h, w, 3), dtype))[..., c] = np.clip(np.floor(v + 0.5), 0, max_value)
                v = np.mean([synth.sample_bilinear(texs[c], (t[0], t[1], t[2] + s * np.cos(angle), t[3] + s * np.sin(angle)), w, h, margin)
                             for s in taps], axis=0)
            v = v + rng.normal(0, noise * max_value / 255.0, v.shape)
            frames[i, :, :, c] = np.clip(np.floor(v + 0.5), 0, max_value)
    return frames, truth, path
