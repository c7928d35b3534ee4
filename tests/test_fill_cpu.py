"""-m "not gpu": the border-fill rule's reference (tests/_fill_ref.py) checked against known answers, and the new public symbols.

Nothing of the GPU code is in the first three tests: they establish that the reference the GPU tests compare against is the rule, that
"covered" means what it says, and that the engine's candidate transforms point the right way."""
import ctypes

import numpy as np

import _engine_model as EM
import _fill_ref as R


def test_known_answer_integer_translations(oracle):
    """frames cut from one large texture at integer offsets, candidates with the matching integer translations: wherever a candidate
    covers, the result IS the texture at the output's position; where none does, candidate 0's border"""
    O = oracle
    rng = np.random.default_rng(3)
    w, h = 96, 64
    for dtype, maxv in ((np.uint8, 255), (np.uint16, 1023)):
        tex = rng.integers(0, maxv + 1, (260, 300, 3)).astype(dtype)
        offs = [(100, 90), (93, 95), (108, 84), (100, 101), (87, 80)]                   # (ox, oy) of frame i in the texture
        src = np.stack([tex[oy:oy + h, ox:ox + w] for ox, oy in offs])
        for (px, py), order in (((96, 88), [0, 1, 2, 3, 4]), ((104, 97), [0, 3, 2, -1, 1]), ((100, 90), [0, 1, 2, 3, 4]), ((91, 99), [2, 2, 1, 4, 0])):
            # frame i shows tex[oy + y, ox + x]; the output at (px, py) wants tex[py + y, px + x] = frame_i[y + py - oy, x + px - ox]: forward shift o - p
            ts = [O.Transform.of(0, 0, offs[max(i, 0)][0] - px, offs[max(i, 0)][1] - py) for i in order]
            want = tex[py:py + h, px:px + w]
            for border in (O.BORDER_CONSTANT, O.BORDER_CLAMP):
                out, cov0, still_open = R.fill_frame(O, src, order, ts, border, maxv, want_masks=True)
                assert (~still_open).sum() > cov0.sum() or cov0.all()                   # the candidates add something
                assert np.array_equal(out[~still_open], want[~still_open])
                plain = O.bgr_image_warp(src[order[0]], ts[0], O.WARP_BILINEAR_CV, border=border, max_value=maxv)
                assert np.array_equal(out[still_open], plain[still_open])
                # the expected coverage, from the geometry alone: candidate i sees output pixel (x, y) iff its four taps are inside frame i
                ys, xs = np.mgrid[0:h, 0:w]
                seen = np.zeros((h, w), bool)
                for i in order:
                    if i < 0:
                        break
                    sx, sy = xs + px - offs[i][0], ys + py - offs[i][1]
                    seen |= (sx >= 0) & (sx + 1 <= w - 1) & (sy >= 0) & (sy + 1 <= h - 1)
                assert np.array_equal(seen, ~still_open)


def test_covered_pixels_are_border_free(oracle):
    O = oracle
    rng = np.random.default_rng(5)
    for dtype, maxv, (w, h) in ((np.uint8, 255, (131, 77)), (np.uint16, 1023, (90, 120))):
        src = rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)
        n_cov = 0
        for tr in [(0.01, -0.02, 7.3, -4.6), (-0.03, 0.015, -11.2, 6.1), (0, 0, 0.5, 0.5), (0.2, 0.1, 30.0, 20.0), (0, 0, 500.0, 0)]:
            t = O.Transform.of(*tr)
            cov = R.covered(O, t, w, h)
            a = O.bgr_image_warp(src, t, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=maxv)
            b = O.bgr_image_warp(src, t, O.WARP_BILINEAR_CV, border=O.BORDER_CLAMP, max_value=maxv)
            assert np.array_equal(a[cov], b[cov])
            n_cov += int(cov.sum())
            if tr[2] == 500.0:
                assert not cov.any()
        assert n_cov > 0


def test_candidate_chain_direction(oracle):
    """make_clip(320, 240, 40, seed=5), 4 frames ahead, crop 0, against the same scene rendered 64 px wider on every side: the mean error on
    filled pixels is below half of what the reference gives with the motion chain un-inverted, and at least 85 % of the uncovered pixels are
    filled.  (Measured when this was written: 1.73 LSB against 11.4, 92.6 % filled.)"""
    from video_stabilizer_amd import synth
    O = oracle
    W, H, N, P, seed = 320, 240, 40, 64, 5
    small, path = synth.make_clip(W, H, N, seed, channels=3)
    big, _ = synth.make_clip(W + 2 * P, H + 2 * P, N, seed, channels=3, path=path, margin=128 - P)
    assert np.array_equal(big[:, P:-P, P:-P], small)

    def run(flip):
        st = O.Stabilizer(crop_pixels=0, lag=10)
        accum = {}
        for i in range(N):
            if st.process(small[i]) is not None:
                accum[i - 10] = O.Transform.of(*st.state()[1].tup())
        m = EM.engine_model(O, small, fill=4, flip=flip, want_masks=True, crop_pixels=0, lag=10)
        assert sorted(m.outs) == sorted(accum)
        errs, unc, filled = [], 0, 0
        for k, out in m.outs.items():
            cov0, still_open = m.masks[k]
            truth = O.bgr_image_warp(big[k], O.t_inverse(accum[k]), O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT)[P:-P, P:-P]
            fm = ~cov0 & ~still_open
            unc += int((~cov0).sum())
            filled += int(fm.sum())
            if fm.any():
                errs.append(np.abs(out.astype(np.int64) - truth.astype(np.int64))[fm].mean())
        return float(np.mean(errs)), filled / max(unc, 1), unc
    e_ok, share_ok, unc = run(False)
    e_flip, share_flip, _ = run(True)
    print("uncovered px %d; filled %.1f %% at %.2f LSB; chain un-inverted: %.1f %% at %.2f LSB" % (unc, 100 * share_ok, e_ok, 100 * share_flip, e_flip))
    assert unc > 0
    assert e_ok < 0.5 * e_flip
    assert share_ok >= 0.85


def test_library_exports_the_fill_symbols(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_bgr_image_warp_fill_batch", "vs_stabilizer_set_border_fill", "vs_stabilizer_get_border_fill"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
