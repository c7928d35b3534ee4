"""-m "not gpu": the inpaint rule's two restatements (tests/_inpaint_ref.py, vectorised; tests/_inpaint_direct.py, pixel by pixel) held against
each other, against a hand-computed case and against the rule's five consequences; what the pass is worth on the border fill's own scene;
the new public symbols.  Nothing of the GPU code runs here: these tests establish that what the GPU tests compare against is the rule."""
import ctypes

import numpy as np
import pytest

import _engine_model as EM
import _fill_ref as F
import _inpaint_direct as D
import _inpaint_ref as R

SIZES = [(1, 1), (2, 2), (1, 9), (9, 1), (3, 5), (65, 33), (130, 70)]      # (w, h)


def _case(rng, w, h, kept, dtype=np.uint8, maxv=255):
    img = rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)
    mask = (rng.random((h, w)) < kept).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)     # any non-zero byte keeps
    return img, mask


@pytest.mark.parametrize("w,h", SIZES)
def test_the_two_restatements_agree(w, h):
    rng = np.random.default_rng(1000 * w + h)
    for kept in (0.02, 0.5, 0.98):
        for dtype, maxv in ((np.uint8, 255), (np.uint16, 65535)):
            img, mask = _case(rng, w, h, kept, dtype, maxv)
            a, b = R.inpaint(img, mask), D.inpaint(img, mask)
            assert a.dtype == img.dtype and np.array_equal(a, b), (w, h, kept, dtype)


def test_hand_computed_4x4():
    """kept: (0,0) = 10, (1,0) = 20, (0,1) = 40, (3,3) = 200.  Level 1: (0,0) = (2 * 70 + 3) // 6 = 23, (1,1) = 200, the other two undefined;
    level 2: (2 * 223 + 2) // 4 = 112; level 1 pulled from it: 112 in both undefined texels (all four taps are the one texel).  Level 0
    from P = [[23, 112], [112, 200]]: e.g. pixel (2,0): px = 1, qx = 0, py = qy = 0: (9 * 112 + 3 * 23 + 3 * 112 + 23 + 8) >> 4 = 1444 >> 4 = 90;
    pixel (1,1): px = 0, qx = 1, py = 0, qy = 1: (9 * 23 + 3 * 112 + 3 * 112 + 200 + 8) >> 4 = 1087 >> 4 = 67."""
    mask = np.array([[1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 9]], np.uint8)
    junk = 231
    c0 = np.array([[10, 20, junk, junk], [40, junk, junk, junk], [junk] * 4, [junk, junk, junk, 200]], np.uint8)
    img = np.stack([c0, c0, np.where(mask != 0, 7, junk).astype(np.uint8)], -1)
    want0 = np.array([[10, 20, 90, 112], [40, 67, 112, 134], [90, 112, 156, 178], [112, 134, 178, 200]], np.uint8)
    want = np.stack([want0, want0, np.full((4, 4), 7, np.uint8)], -1)
    assert np.array_equal(R.inpaint(img, mask), want)
    assert np.array_equal(D.inpaint(img, mask), want)


@pytest.mark.parametrize("inpaint", [R.inpaint, D.inpaint], ids=["ref", "direct"])
def test_consequences(inpaint):
    rng = np.random.default_rng(9)
    for (w, h), dtype, maxv in (((37, 21), np.uint8, 255), ((20, 33), np.uint16, 1023)):
        for kept in (0.02, 0.5, 0.98):
            img, mask = _case(rng, w, h, kept, dtype, maxv)
            if not mask.any():
                mask[h // 2, w // 2] = 1
            out = inpaint(img, mask)
            keep = mask != 0
            assert np.array_equal(out[keep], img[keep])                                        # (a)
            for c in range(3):                                                                 # (b)
                assert out[..., c].min() >= img[..., c][keep].min() and out[..., c].max() <= img[..., c][keep].max()
            flat = img.copy()                                                                  # (c)
            flat[keep] = (5, 250 % (maxv + 1), maxv)
            assert (inpaint(flat, mask) == np.array((5, 250 % (maxv + 1), maxv), dtype)).all()
            assert np.array_equal(inpaint(img, np.ones_like(mask)), img)                       # (d)
            assert np.array_equal(inpaint(img, np.zeros_like(mask)), img)
            other = np.where(keep[..., None], img, rng.integers(0, maxv + 1, img.shape).astype(dtype))     # (e)
            assert np.array_equal(inpaint(other, mask), out)
            assert np.array_equal(inpaint(np.where(keep[..., None], img, maxv).astype(dtype), mask), out)


def test_coverage_index_is_the_fill_references_open_set(oracle):
    O = oracle
    rng = np.random.default_rng(4)
    w, h, n_src = 96, 64, 5
    src = rng.integers(1, 256, (n_src, h, w, 3)).astype(np.uint8)
    for order in ([0, 1, 2, 3, 4], [2, 3, -1, 1, 0], [4]):
        ts = [O.Transform.of(rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-25, 25), rng.uniform(-20, 20)) for _ in order]
        for roi in (None, (7, 5, 64, 40)):
            cov = R.coverage_frame(O, order, ts, w, h, roi)
            _, cov0, open_ = F.fill_frame(O, src, order, ts, O.BORDER_CONSTANT, 255, roi, want_masks=True)
            assert np.array_equal(cov != 0, ~open_) and np.array_equal(cov == 1, cov0)
            live = order[:order.index(-1)] if -1 in order else order
            assert cov.max() <= len(live)
    # candidate 0 far away, candidate 1 the identity: its right tap / lower tap leaves the frame in the last column / row
    cov = R.coverage_frame(O, [0, 1], [O.Transform.of(0, 0, 500, 0), O.Transform.of()], w, h)
    assert (cov[:-1, :-1] == 2).all() and not cov[-1].any() and not cov[:, -1].any()


def test_quality_on_the_fills_own_scene(oracle):
    """make_clip(320, 240, 40, seed=5), 4 frames ahead, crop 0, against the same scene rendered 64 px wider on every side (the scene of
    tests/test_fill_cpu.py): the mean absolute error of the samples that stay open behind the fill, after inpainting, is below what the
    constant border leaves there.  (Measured when this was written: 8211 still-open samples; inpaint 7.65 levels, constant border 96.69, clamp border
    6.23 -- on this smooth scene the clamp border's smear is as good a guess; the inpaint serves the default constant border.)"""
    from video_stabilizer_amd import synth
    O = oracle
    W, H, N, P, seed = 320, 240, 40, 64, 5
    small, path = synth.make_clip(W, H, N, seed, channels=3)
    big, _ = synth.make_clip(W + 2 * P, H + 2 * P, N, seed, channels=3, path=path, margin=128 - P)
    st = O.Stabilizer(crop_pixels=0, lag=10)
    accum = {}
    for i in range(N):
        if st.process(small[i]) is not None:
            accum[i - 10] = O.Transform.of(*st.state()[1].tup())
    const = EM.engine_model(O, small, fill=4, want_masks=True, crop_pixels=0, lag=10, warp_border=O.BORDER_CONSTANT)
    clamp = EM.engine_model(O, small, fill=4, want_masks=True, crop_pixels=0, lag=10, warp_border=O.BORDER_CLAMP)
    err = {"inpaint": 0, "constant": 0, "clamp": 0}
    n_open = 0
    for k, out in const.outs.items():
        still_open = const.masks[k][1]
        truth = O.bgr_image_warp(big[k], O.t_inverse(accum[k]), O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT)[P:-P, P:-P].astype(np.int64)
        assert np.array_equal(still_open, clamp.masks[k][1])
        n_open += 3 * int(still_open.sum())
        for name, res in (("inpaint", R.inpaint(out, ~still_open)), ("constant", out), ("clamp", clamp.outs[k])):
            err[name] += int(np.abs(res.astype(np.int64) - truth)[still_open].sum())
    assert n_open > 0
    mae = {k: v / n_open for k, v in err.items()}
    print("still-open samples %d; mean absolute error: inpaint %.2f, constant border %.2f, clamp border %.2f" % (n_open, mae["inpaint"], mae["constant"], mae["clamp"]))
    assert mae["inpaint"] < mae["constant"]


def test_premises_of_the_hostile_cases(oracle):
    """every builder of tests/_inpaint_cases.py asserts its premise (what makes its input reach the code in question) on the references
    alone; the shapes and formats are those of tests/test_inpaint_hostile_gpu.py"""
    import _inpaint_cases as IC
    O = oracle
    for w, h in ((300, 270), (520, 70)):
        for n_cand in (5, 16):
            IC.rotation_case(O, w, h, n_cand)
        IC.rotation_rois(w, h)
    IC.hostile_case(O)
    IC.nothing_covered_cases(O)
    IC.sixteen_case(O)
    for n_cand, extra in ((16, 3), (1, 1)):
        IC.seam_case(O, n_cand, extra)
    for fmt in ("u8", "bgr10", "bgr16"):
        for w, h in ((63, 65), (300, 270)):
            for high in (0, 1):
                for open_share in (0.5, 0.9):
                    IC.rounding_case(w, h, fmt, high, open_share)
    for fmt in ("bgr10", "bgr12"):
        for w, h in ((131, 77), (300, 270)):
            IC.out_of_range_case(w, h, fmt)
    for fmt in ("u8", "bgr16"):
        for w, h in ((300, 270), (60, 50)):
            IC.idle_and_busy_batch(w, h, fmt)
    # the 2 x 2 closed form is the rule on every mask pattern
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (16, 2, 2, 3)).astype(np.uint8)
    masks = np.array([[(k >> b) & 1 for b in range(4)] for k in range(16)], np.uint8).reshape(16, 2, 2) * 0x80
    assert np.array_equal(IC.inpaint_2x2(imgs, masks), R.inpaint_batch(imgs, masks))
    # the windowed coverage is the rule's, cropped
    for t in ((0.02, -0.03, 7.0, -5.0), IC.ZOOM_IN, (-1 + 1e-9, 1e-9, 3.0, 2.0), (0.0, 0.0, 6e5, 0.0)):
        for roi in ((0, 0, 64, 48), (5, 7, 20, 11), (63, 47, 1, 1)):
            cov, _ = IC.covered_window(O, O.Transform.of(*t), 64, 48, roi)
            assert np.array_equal(cov, F.covered(O, O.Transform.of(*t), 64, 48)[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]])


def test_the_tails_lds_holds_every_shape_it_is_given():
    """vs_inpaint.hip's make_plan starts the tail at the first level of at most 4096 texels (kTailTexels); the tail keeps that level and all
    below it in 8192 texels of LDS (kTailLds).  Enumerated: over every W x H <= 4096 the levels from there down sum to at most 8191, reached at
    1 x 4096 and 4096 x 1 -- so the plan's second condition never moves the tail, and the shapes of tests/test_inpaint_hostile_gpu.py hold the
    maximum"""
    def below(w, h):
        t = w * h
        while w > 1 or h > 1:
            w, h = (w + 1) >> 1, (h + 1) >> 1
            t += w * h
        return t
    worst = max((below(w, h), w, h) for w in range(1, 4097) for h in range(1, 4096 // w + 1))
    assert worst[0] == 8191 and {(w, h) for w in range(1, 4097) for h in range(1, 4096 // w + 1) if below(w, h) == 8191} == {(1, 4096), (4096, 1)}


def test_library_exports_the_inpaint_symbols(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_bgr_fill_coverage_batch", "vs_bgr_inpaint_batch", "vs_stabilizer_set_inpaint", "vs_stabilizer_get_inpaint"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
