"""-m "not gpu": the deblur rule's restatement (tests/_deblur_ref.py) checked for the rule's exact consequences and for the direction and
centre of the engine's candidate maps, and the new public symbols.

Nothing of the GPU code is in the first five tests (the host algebra's cv_inverse_matrix is): they establish that the reference the GPU
tests compare against is the rule and that the engine model's maps point the right way, before a kernel is involved."""
import ctypes

import numpy as np

import _deblur_ref as R
import _engine_model as EM


def _cvinv(vs):
    return lambda t, w, h: vs.cv_inverse_matrix(vs.Transform.of(*t.tup()), w, h)


def _T(vs, *a):
    return vs.Transform.of(*a)


def test_sharpness_known_answers():
    """a horizontal ramp of slope 3: every interior pixel has gx = 6, gy = 0; a checkerboard of 0 / 255 has central differences 0"""
    w, h = 21, 13
    ramp = np.repeat((np.arange(w) * 3)[None, :, None], h, 0).repeat(3, 2).astype(np.uint8)
    assert R.sharpness(ramp, 8) == 36 * (w - 2) * (h - 2)
    yy, xx = np.mgrid[0:h, 0:w]
    check = (((xx + yy) & 1) * 255)[..., None].repeat(3, 2).astype(np.uint8)
    assert R.sharpness(check, 8) == 0
    stripes = ((xx // 2 & 1) * 255)[..., None].repeat(3, 2).astype(np.uint8)            # period 4: |g(x+1) - g(x-1)| = 255 everywhere
    assert R.sharpness(stripes, 8) == 255 * 255 * (w - 2) * (h - 2)
    assert R.sharpness(np.zeros((2, 9, 3), np.uint8), 8) == 0
    # 10-bit samples: the gray is shifted to 8 bits first
    ramp10 = (ramp.astype(np.uint16) * 4)
    assert R.sharpness(ramp10, 10) == R.sharpness(ramp, 8)
    # the bound of the header: 130050 per pixel
    assert 2 * 255 * 255 == 130050 and 130050 * 65535 * 65535 < 2 ** 53


def test_three_identities(vs):
    """no sharper candidate, identical frames (ties on S), n_cand == 1: the target comes back bit for bit"""
    rng = np.random.default_rng(1)
    cv = _cvinv(vs)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 10), (np.uint16, 16)):
        maxv = (1 << bits) - 1
        sharp_f = rng.integers(0, maxv + 1, (40, 56, 3)).astype(dtype)
        soft = (sharp_f.astype(np.int64) // 8 + maxv // 3).astype(dtype)                  # the same picture at an eighth of the contrast
        src = np.stack([sharp_f, soft, sharp_f, soft])
        S = R.sharpness_batch(src, bits)
        assert S[0] == S[2] > S[1] == S[3]
        ts = [_T(vs), _T(vs, 0.01, -0.02, 1.5, -2.0), _T(vs, 0, 0, 3, 1), _T(vs)]
        # the sharpest frame of its window
        assert np.array_equal(R.deblur_frame(cv, src, S, [0, 1, 3, 2], ts, bits, maxv), src[0])
        # ties
        assert np.array_equal(R.deblur_frame(cv, src, S, [0, 2, 2, 2], ts, bits, maxv), src[0])
        assert np.array_equal(R.deblur_frame(cv, src, S, [1, 3, 3, -1], ts, bits, maxv), src[1])
        # one candidate
        assert np.array_equal(R.deblur_frame(cv, src, S, [1], ts[:1], bits, maxv), src[1])
        # a negative index ends the list in front of the sharper frame
        assert np.array_equal(R.deblur_frame(cv, src, S, [1, -1, 0, 0], ts, bits, maxv), src[1])
        # and the soft frame does change when the sharp one takes part
        assert not np.array_equal(R.deblur_frame(cv, src, S, [1, 0, -1, -1], ts, bits, maxv), src[1])


def test_max_ratio_is_honoured(vs):
    """a black target (S_k = 0) keeps at least 1 / (1 + n max_ratio^2 / sensitivity) of its own weight: with white candidates the output is
    at most 255 (1 - that share), whatever their sharpness"""
    cv = _cvinv(vs)
    rng = np.random.default_rng(2)
    h, w = 24, 32
    black = np.zeros((h, w, 3), np.uint8)
    busy = rng.integers(0, 2, (h, w, 1)).astype(np.uint8).repeat(3, 2) * 255
    for n in (1, 4, 15):
        for max_ratio, sens in ((4.0, 2.0), (1.5, 0.5), (100.0, 8.0)):
            src = np.stack([black] + [busy] * n)
            S = R.sharpness_batch(src, 8)
            assert S[0] == 0 and S[1] > 0
            out, W = R.deblur_frame(cv, src, S, list(range(n + 1)), [_T(vs)] * (n + 1), 8, 255, sens, max_ratio, want_weight=True)
            share = 1.0 / (1.0 + n * max_ratio ** 2 / sens)
            assert (1.0 / W.astype(np.float64)).min() >= share * (1 - 1e-6)
            assert out.max() <= np.ceil(255 * (1 - share) + 0.5)
            # where the candidates are black too, d = 0 and the weight is exactly the bound
            assert np.isclose(W.max(), 1 + n * max_ratio ** 2 / sens, rtol=1e-6)


def test_out_of_frame_samples_contribute_nothing(vs):
    cv = _cvinv(vs)
    rng = np.random.default_rng(4)
    h, w = 30, 44
    sharp_f = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    soft = (sharp_f // 8 + 90).astype(np.uint8)
    src = np.stack([soft, sharp_f])
    S = R.sharpness_batch(src, 8)
    # the candidate lies 10 px to the right and 7 px down: target (x, y) is its pixel (x - 10, y - 7)
    out, W = R.deblur_frame(cv, src, S, [0, 1], [_T(vs), _T(vs, 0, 0, 10, 7)], 8, 255, want_weight=True)
    assert np.array_equal(out[:7], soft[:7]) and np.array_equal(out[:, :10], soft[:, :10])
    assert (W[:7] == 1).all() and (W[:, :10] == 1).all() and (W[7:, 10:] > 1).all()
    # entirely outside: a copy, although the candidate takes part
    assert np.array_equal(R.deblur_frame(cv, src, S, [0, 1], [_T(vs), _T(vs, 0, 0, 500, 0)], 8, 255), soft)
    # integer shift, known answer: the blend of soft(x, y) and sharp(x - 10, y - 7) by the rule's weights in float64
    gk = R.gray8(soft, 8)[7:, 10:].astype(np.float64)
    gj = R.gray8(sharp_f, 8)[:h - 7, :w - 10].astype(np.float64)
    r = min(float(S[1]) / float(S[0]), 4.0)
    wt = r * r / (np.abs(gk - gj) + 2.0)
    want = (soft[7:, 10:].astype(np.float64) + wt[..., None] * sharp_f[:h - 7, :w - 10]) / (1 + wt[..., None])
    assert np.abs(out[7:, 10:].astype(np.float64) - want).max() <= 0.5 + 1e-3


CLIP = dict(w=320, h=240, n=20, seed=11, blurred=(4,), jitter_b=0.03)


def test_direction_and_centre_of_the_engine_maps(vs, oracle):
    """blurred_clip(320 x 240, 20 frames, seed 11, rotation jitter 0.03 rad so that the centre matters, 1 LSB noise, frame 4 blurred along
    6 px), maps from the CPU oracle's measured transforms, four frames ahead.  The mean error against the unblurred render of frame 4, as a
    share of the input frame's error: the right maps must cut it to at most 1.25 x the value measured when this was written and to under
    0.7 in any case; the chain un-inverted (the wrong direction) must not cut it at all, and the transforms applied about pixel (0, 0)
    instead of the frame's centre must not reach 0.7.  ("The other centre" is the corner: half a pixel of centre -- (w/2, h/2) against
    ((w-1)/2, (h-1)/2) -- moves a sample by |B| / 2 < 0.02 px on this clip, which no nearest-sample test can see.)
    Measured when this was written: input error 3.24 LSB; right 0.527; wrong direction 1.510; corner 0.913."""
    from video_stabilizer_amd import synth
    O = oracle
    frames, truth, _ = R.blurred_clip(synth, **CLIP)
    k = CLIP["blurred"][0]
    meas, succ, due, _ = EM.measure(O, frames, lag=10, crop_pixels=0)
    assert all(succ[k + 1:k + 5])
    S = R.sharpness_batch(frames, 8)
    assert all(S[j] > S[k] for j in range(k + 1, k + 5))
    e_in = np.abs(frames[k].astype(np.float64) - truth[k]).mean()

    def corner(t, w, h):
        M = np.linalg.inv(np.array([[1 + t.A, -t.B, t.TX], [t.B, 1 + t.A, t.TY], [0, 0, 1]]))
        return M[:2].reshape(6)

    def ratio(mode, cvinv):
        cf, ct = EM.lookahead_candidates(O, k, 4, meas, succ, mode)
        d = R.deblur_frame(cvinv, frames, S, cf, ct, 8, 255)
        return np.abs(d.astype(np.float64) - truth[k]).mean() / e_in
    right, flip, other = ratio("right", _cvinv(vs)), ratio("flip", _cvinv(vs)), ratio("right", corner)
    print("input error %.2f LSB; right maps %.3f, wrong direction %.3f, corner centre %.3f of it" % (e_in, right, flip, other))
    assert right <= min(1.25 * 0.527, 0.7)
    assert flip >= 1.0
    assert other > 0.7
    # the sharpest frame of its window comes back bit for bit
    ks = max(range(1, 10), key=lambda j: int(S[j]))
    cf, ct = EM.lookahead_candidates(O, ks, 4, meas, succ)
    if all(S[j] <= S[ks] for j in cf[1:] if j >= 0):
        assert np.array_equal(R.deblur_frame(_cvinv(vs), frames, S, cf, ct, 8, 255), frames[ks])


def test_library_exports_the_deblur_symbols(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_deblur_params_default", "vs_bgr_sharpness_batch", "vs_bgr_deblur_batch", "vs_stabilizer_set_deblur", "vs_stabilizer_get_deblur"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
    p = vs.deblur_params()
    assert (p.sensitivity, p.max_ratio) == (2.0, 4.0)
