"""-m "not gpu": the fill's blend rule as restated in tests/_fill_blend_ref.py, checked against the rule's stated consequences, known answers
and a hand-computed ramp; a quality pin on a clip with exposure drift; the new public symbols.

Nothing of the GPU code is in the tests but the last: they establish that the reference the GPU tests compare against is the rule."""
import ctypes

import numpy as np

import _engine_model as EM
import _fill_blend_ref as B
import _fill_ref as R


def _frames(rng, n, w, h, dtype, maxv):
    base = rng.integers(0, maxv + 1, (n, h // 8 + 2, w // 8 + 2, 3))
    up = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :h, :w]
    return np.clip(up + rng.integers(-3, 4, up.shape), 0, maxv).astype(dtype)


def _case(O, rng, dtype, maxv, w=97, h=71, n_src=4):
    src = _frames(rng, n_src, w, h, dtype, maxv)
    src[1] = np.clip(src[1].astype(np.int64) * 5 // 4, 0, maxv).astype(dtype)        # exposure differs from frame to frame
    src[2] = (src[2].astype(np.int64) * 3 // 4).astype(dtype)
    own = (0.02, -0.03, 9.3, -6.7)
    ct = [O.Transform.of(*own)] + [O.Transform.of(own[0] + rng.uniform(-0.02, 0.02), own[1] + rng.uniform(-0.02, 0.02),
                                                  own[2] + rng.uniform(-8, 8), own[3] + rng.uniform(-8, 8)) for _ in range(n_src - 1)]
    return src, list(range(n_src)), ct, B.channel_sums(src)


def test_consequences_of_the_rule(oracle):
    O = oracle
    rng = np.random.default_rng(41)
    for dtype, maxv in ((np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)):
        src, cf, ct, sums = _case(O, rng, dtype, maxv)
        _, h, w, _ = src.shape
        for border in (O.BORDER_CONSTANT, O.BORDER_CLAMP):
            plain = O.bgr_image_warp(src[0], ct[0], O.WARP_BILINEAR_CV, border=border, max_value=maxv)
            # (a) both switches off: the fill
            assert np.array_equal(B.blend_frame(O, src, cf, ct, sums, 0, 0, border, maxv), R.fill_frame(O, src, cf, ct, border, maxv))
            nowhere = [O.Transform.of(0.0, 0.0, 5000.0, -3000.0)] + ct[1:]
            assert not R.covered(O, nowhere[0], w, h).any()
            for feather in (0, 1, 4, 6):
                for match in (0, 1):
                    # (b) no later candidate: the plain warp
                    assert np.array_equal(B.blend_frame(O, src, cf[:1], ct[:1], sums, feather, match, border, maxv), plain)
                    assert np.array_equal(B.blend_frame(O, src, [0, -1, -1, -1], ct, sums, feather, match, border, maxv), plain)
                    out, cov0, still_open, band = B.blend_frame(O, src, cf, ct, sums, feather, match, border, maxv, want_masks=True)
                    # (c) a band pixel lies between the plain value and the matched fill sample (the latter: what the same candidates give where
                    # candidate 0 covers nothing)
                    f = B.blend_frame(O, src, cf, nowhere, sums, 0, match, border, maxv)
                    assert band.any() == (feather > 0)
                    lo, hi = np.minimum(plain, f)[band], np.maximum(plain, f)[band]
                    assert ((out[band] >= lo) & (out[band] <= hi)).all()
                    assert np.array_equal(out[still_open], plain[still_open])
                    assert np.array_equal(out[~cov0 & ~still_open], f[~cov0 & ~still_open])
                    # (e) at least 2^feather source pixels inside candidate 0's frame: never changed
                    sx, sy = R.cv_source_ints(O, ct[0], w, h)
                    m = 1 << feather
                    deep = (sx >= m) & (sx + 1 <= w - 1 - m) & (sy >= m) & (sy + 1 <= h - 1 - m)
                    assert deep.any() or feather == 6
                    assert np.array_equal(out[deep], plain[deep])
                    assert not (band & deep).any()
        # (d) identical frames under identity maps: bit for bit with any setting
        same = np.stack([src[0]] * 3)
        ident = [O.Transform.of()] * 3
        for feather in (0, 3, 6):
            for match in (0, 1):
                assert np.array_equal(B.blend_frame(O, same, [0, 1, 2], ident, B.channel_sums(same), feather, match, O.BORDER_CONSTANT, maxv),
                                      O.bgr_image_warp(src[0], ident[0], O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=maxv))


def test_gain_known_answers():
    assert B.gain_q15(12345, 12345) == 32768                          # equal sums
    assert B.gain_q15(0, 999) == 32768 and B.gain_q15(999, 0) == 32768 and B.gain_q15(0, 0) == 32768
    assert B.gain_q15(3000, 1000) == 65536 and B.gain_q15(2001, 1000) == 65536       # beyond 2: clamped
    assert B.gain_q15(2000, 1000) == 65536 and B.gain_q15(1999, 1000) == 65503       # (32768 * 1.999 = 65503.2)
    assert B.gain_q15(1000, 3000) == 16384 and B.gain_q15(1000, 2001) == 16384       # below 1/2: clamped
    assert B.gain_q15(3, 4) == 24576 and B.gain_q15(5, 4) == 40960                   # exact ratios
    # the rounded division's tie goes up: 32768 * 40001 / 65536 = 20000.5
    assert B.gain_q15(40001, 65536) == 20001
    assert B.gain_q15(39999, 65536) == 20000                                          # 19999.5
    # the largest sums the rule admits stay inside 2^63
    big = 65535 * 32767 * 32767
    assert big < 1 << 46 and B.gain_q15(big, big) == 32768 and B.gain_q15(big, big // 2 + 1) == 65536
    # a 16-bit sample of 65535 at gain 65536 saturates without wrapping: the product stays below 2^32
    assert 65535 * 65536 + 16384 < 1 << 32
    assert B.matched(np.array([[65535, 65535, 1]]), [65536, 32768, 65536], 65535).tolist() == [[65535, 65535, 2]]
    assert B.matched(np.array([[1023, 600, 0]]), [65536, 65536, 65536], 1023).tolist() == [[1023, 1023, 0]]
    assert B.matched(np.array([[200, 201, 7]]), [16384, 16384, 16384], 255).tolist() == [[100, 101, 4]]      # 100.5 + .5 -> 101; 3.5 + .5 -> 4


def test_hand_computed_ramp(oracle):
    """candidate 0: a constant frame of 100 shifted right by 5 pixels; candidate 1: a constant frame of 200, unshifted; feather 2 (K = 128: four source
    pixels).  24 x 24, row 12 (Y = 384, Ymax - Y = 351: the rows' distance plays no part).  Output pixel x samples candidate 0 at sx = x - 5: X =
    32 (x - 5), covered for 5 <= x <= 23; Xmax = 735.  k = X + 1 = 1, 33, 65, 97 at x = 5 .. 8, 129 >= K from x = 9; at x = 23, Xmax - X = 159 >= K.
        x = 0 .. 4   uncovered, candidate 1 covers                  200
        x = 5        (1 * 100 + 127 * 200 + 64) >> 7 = 25564 >> 7    199
        x = 6        (33 * 100 + 95 * 200 + 64) >> 7 = 22364 >> 7    174
        x = 7        (65 * 100 + 63 * 200 + 64) >> 7 = 19164 >> 7    149
        x = 8        (97 * 100 + 31 * 200 + 64) >> 7 = 15964 >> 7    124
        x = 9 .. 23  plain                                           100
    With match on, G = (65536 * 100 + 200) // 400 = 16384 and f = (200 * 16384 + 16384) >> 15 = 100: the whole row is 100."""
    O = oracle
    w = h = 24
    for dtype, maxv in ((np.uint8, 255), (np.uint16, 1023)):
        src = np.stack([np.full((h, w, 3), 100, dtype), np.full((h, w, 3), 200, dtype)])
        ct = [O.Transform.of(0, 0, 5, 0), O.Transform.of(0, 0, 0, 0)]
        sums = B.channel_sums(src)
        assert sums.tolist() == [[100 * w * h] * 3, [200 * w * h] * 3]
        out = B.blend_frame(O, src, [0, 1], ct, sums, 2, 0, O.BORDER_CONSTANT, maxv)
        row = [200] * 5 + [199, 174, 149, 124] + [100] * 15
        assert out[12, :, 0].tolist() == row and out[12, :, 1].tolist() == row and out[12, :, 2].tolist() == row
        assert B.blend_frame(O, src, [0, 1], ct, sums, 0, 0, O.BORDER_CONSTANT, maxv)[12, :, 1].tolist() == [200] * 5 + [100] * 19
        assert B.gain_q15(sums[0][0], sums[1][0]) == 16384
        assert (B.blend_frame(O, src, [0, 1], ct, sums, 2, 1, O.BORDER_CONSTANT, maxv)[12] == 100).all()
        # a shift up by 3 rows instead: the same ramp runs down a column from the bottom edge (Y = 32 (y + 3), Ymax - Y = 735 - 32 (y + 3))
        ct = [O.Transform.of(0, 0, 0, -3), O.Transform.of(0, 0, 0, 0)]
        out = B.blend_frame(O, src, [0, 1], ct, sums, 2, 0, O.BORDER_CONSTANT, maxv)
        # y = 19: sy = 22, Y = 704, Ymax - Y = 31, k = 32: (32 * 100 + 96 * 200 + 64) >> 7 = 175;  y = 18: k = 64: (6400 + 12800 + 64) >> 7 = 150;
        # y = 17: k = 96: (9600 + 6400 + 64) >> 7 = 125;  y = 16: k = 128: plain;  y = 20 .. 22: uncovered, candidate 1 covers (sy <= 22); y = 23: border;
        # and at the top y = 0: Y = 96, k = 97: (9700 + 6200 + 64) >> 7 = 124;  y = 1: Y = 128, k = 129: plain
        assert out[:, 12, 2].tolist() == [124] + [100] * 16 + [125, 150, 175] + [200] * 3 + [0]


def test_quality_pin_exposure_drift(oracle):
    """make_clip(320, 240, 40, seed=5), 4 frames ahead, crop 0, the same scene rendered 64 px wider as ground truth (the clip of
    tests/test_fill_cpu.py::test_candidate_chain_direction), every frame multiplied by a smooth exposure factor within +-10 %; the transforms are
    those of the UNSCALED clip.  Measured when this was written (mean absolute error on filled pixels against the truth at frame k's exposure, 8-bit
    levels): match off 6.35, match on 2.20; mean absolute step across the coverage edge beyond the truth's own step: feather 0 6.24, feather 4 2.02
    (both with match off)."""
    from video_stabilizer_amd import synth
    O = oracle
    W, H, N, P, seed = 320, 240, 40, 64, 5
    small, path = synth.make_clip(W, H, N, seed, channels=3)
    big, _ = synth.make_clip(W + 2 * P, H + 2 * P, N, seed, channels=3, path=path, margin=128 - P)
    gain = 1.0 + 0.1 * np.sin(2 * np.pi * np.arange(N) / 11.0 + 0.7)
    assert gain.min() >= 0.9 and gain.max() <= 1.1 and gain.max() - gain.min() > 0.15

    def expose(clip):
        return np.clip(np.rint(clip.astype(np.float64) * gain[:, None, None, None]), 0, 255).astype(np.uint8)
    dim, dim_big = expose(small), expose(big)
    meas, succ, due, p = EM.measure(O, small, crop_pixels=0, lag=10)
    assert p.warp_mode == O.WARP_BILINEAR_CV and max(p.crop_pixels, 0) == 0
    lists = {k: EM.fill_candidates(O, k, 4, meas, succ, O.t_inverse(acc)) for k, (_, acc) in due.items()}
    border = p.warp_border
    sums = B.channel_sums(dim)
    st = O.Stabilizer(crop_pixels=0, lag=10)
    accum = {}
    for i in range(N):
        if st.process(small[i]) is not None:
            accum[i - 10] = O.Transform.of(*st.state()[1].tup())
    assert sorted(accum) == sorted(lists)
    truth = {k: O.bgr_image_warp(dim_big[k], O.t_inverse(accum[k]), O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT)[P:-P, P:-P].astype(np.int64) for k in lists}

    def run(feather, match):
        errs, steps = [], []
        for k, (cf, ct) in lists.items():
            out, cov0, still_open, _ = B.blend_frame(O, dim, cf, ct, sums, feather, match, border, 255, want_masks=True)
            o, t = out.astype(np.int64), truth[k]
            fm = ~cov0 & ~still_open
            if fm.any():
                errs.append(np.abs(o - t)[fm].mean())
            # neighbouring pixels on either side of the coverage edge, both with a value of the scene (not border)
            known = ~still_open
            for ax in (0, 1):
                a = [slice(None)] * 2
                b = [slice(None)] * 2
                a[ax], b[ax] = slice(0, -1), slice(1, None)
                a, b = tuple(a), tuple(b)
                edge = (cov0[a] != cov0[b]) & known[a] & known[b]
                if edge.any():
                    steps.append(np.abs((o[b] - o[a]) - (t[b] - t[a]))[edge].ravel())
        return float(np.mean(errs)), float(np.concatenate(steps).mean())
    e_off, s_hard = run(0, 0)
    e_on, _ = run(0, 1)
    _, s_soft = run(4, 0)
    print("filled pixels' error: match off %.2f, on %.2f LSB; step across the coverage edge: feather 0 %.2f, feather 4 %.2f LSB" % (e_off, e_on, s_hard, s_soft))
    assert e_on < e_off
    assert s_soft < s_hard


def test_library_exports_the_fill_blend_symbols(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_bgr_channel_sums_batch", "vs_bgr_image_warp_fill_blend_batch", "vs_stabilizer_set_fill_blend", "vs_stabilizer_get_fill_blend"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
    assert ctypes.sizeof(vs.FillBlendParams) == 8
