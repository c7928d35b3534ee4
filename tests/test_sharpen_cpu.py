"""-m "not gpu": the sharpen rule's restatement (tests/_sharpen_ref.py) checked for the rule's consequences (a) to (e), its int32 bound at 16-bit
extremes, a hand-computed 3 x 3 window and a direct float64 form; the defaults, the new public symbols and every argument check that needs no
device; and the premise of DESIGN.md section 28: on a periodic band-limited texture shifted by a sub-pixel phase the sharpened image is closer
to the true shift than the plain warp's, and its gradient energy varies less over the phases.

Nothing here needs a device: the images come from the oracle's plain warp and the restatement."""
import ctypes

import numpy as np
import pytest

import _sharpen_ref as R

FORMATS = ((np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535))


def _noise(rng, h, w, dtype, maxv):
    return rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)


@pytest.mark.parametrize("dtype,maxv", FORMATS)
def test_consequences_a_to_e(vs, dtype, maxv):
    T = vs.Transform.of
    rng = np.random.default_rng(maxv)
    w, h = 37, 29
    img = _noise(rng, h, w, dtype, maxv)
    rot = T(0.03, 0.05, 1.3, -0.7)
    changed = R.sharpen(vs, img, rot, w, h, max_value=maxv)
    assert (changed != img).mean() > 0.3                                 # premise: under a sub-pixel map the rule does something to noise
    # (a) the identity and whole-pixel shifts
    for t in (T(), T(0, 0, 3, -2), T(0, 0, -1, 0)):
        X, Y = R.positions(vs, t, w, h)
        assert not (X & 31).any() and not (Y & 31).any()
        for s in (1, 16, 32):
            assert np.array_equal(R.sharpen(vs, img, t, w, h, strength=s, max_value=maxv), img)
    # (b) a constant image and an image linear in x and y, under any map
    yy, xx = np.mgrid[0:h, 0:w]
    const = np.full((h, w, 3), maxv // 3, dtype)
    lin = np.repeat((3 * xx + 5 * yy + 7)[:, :, None], 3, axis=2).astype(dtype)
    assert lin.max() <= maxv
    for t in (rot, T(0, 0, 0.5, 0.5), T(-0.02, 0.01, 0.25, 0.75)):
        assert np.array_equal(R.sharpen(vs, const, t, w, h, strength=32, max_value=maxv), const)
        assert np.array_equal(R.sharpen(vs, lin, t, w, h, strength=32, max_value=maxv), lin)
    # (c) uncovered pixels and their edge neighbours, and the window's outer ring: a shift that leaves the left and top margins uncovered
    t = T(0, 0, 4.5, 3.5)
    X, Y = R.positions(vs, t, w, h)
    cov = R.covered(X, Y, w, h)
    assert 0.05 < (~cov).mean() < 0.5
    near = ~cov
    near[1:] |= ~cov[:-1]; near[:-1] |= ~cov[1:]; near[:, 1:] |= ~cov[:, :-1]; near[:, :-1] |= ~cov[:, 1:]
    out = R.sharpen(vs, img, t, w, h, max_value=maxv)
    assert np.array_equal(out[near], img[near]) and (out[~near] != img[~near]).any()
    ring = np.ones((h, w), bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(changed[ring], img[ring])
    assert np.array_equal(R.eligible(vs, t, w, h, (0, 0, w, h)), ~near & ~ring)
    # ... the same on a window: its own outer ring, full-frame coordinates for the rest
    roi = (5, 3, 20, 17)
    win = img[3:20, 5:25]
    el = R.eligible(vs, t, w, h, roi)
    assert np.array_equal(el[1:-1, 1:-1], (~near)[4:19, 6:24]) and not el[0].any() and not el[:, 0].any() and not el[-1].any() and not el[:, -1].any()
    ow = R.sharpen(vs, win, t, w, h, roi=roi, max_value=maxv)
    assert np.array_equal(ow[1:-1, 1:-1], out[4:19, 6:24])
    # (d) samples above the format's maximum change only where delta != 0
    if maxv == 1023:
        over = img.copy()
        over[rng.random((h, w)) < 0.2] = 65535
        num = R.numerators(vs, over, rot, w, h)
        o = R.sharpen(vs, over, rot, w, h, max_value=maxv)
        still = ((num + 16384) >> 15) == 0
        assert np.array_equal(o[still], over[still]) and (over[still] > maxv).any()
        assert o[~still].max() <= maxv and (over[~still] > maxv).any()
    # (e) a NaN map (a NaN scale makes every entry of the matrix NaN): X = Y = 0 everywhere
    X, Y = R.positions(vs, T(float("nan"), 0, 0, 0), w, h)
    assert not X.any() and not Y.any() and R.covered(X, Y, w, h).all()
    # ... and maps that are NaN or infinite in part leave every pixel on phase 0 or uncovered
    for t in (T(float("nan"), 0, 0, 0), T(0, 0, float("nan"), 0), T(0, 0, 0, float("inf"))):
        assert np.array_equal(R.sharpen(vs, img, t, w, h, strength=32, max_value=maxv), img)


def test_int32_bound_at_16_bit_extremes(vs):
    """phase (16, 16), strength 32, a 65535 sample among zeros and a zero among 65535s: |num| is the bound itself, and num + 16384 stays in int32"""
    w = h = 8
    t = vs.Transform.of(0, 0, -0.5, -0.5)
    X, Y = R.positions(vs, t, w, h)
    assert ((X & 31) == 16).all() and ((Y & 31) == 16).all()
    hi = np.zeros((h, w, 3), np.uint16)
    hi[3, 3] = 65535
    lo = np.full((h, w, 3), 65535, np.uint16)
    lo[3, 3] = 0
    nh, nl = R.numerators(vs, hi, t, w, h, strength=32), R.numerators(vs, lo, t, w, h, strength=32)
    assert nh.max() == R.NUM_BOUND == 32 * 512 * 131070 and nl.min() == -R.NUM_BOUND
    assert R.NUM_BOUND + 16384 <= 2 ** 31 - 1 and -R.NUM_BOUND + 16384 >= -2 ** 31
    for n in (nh, nl):
        assert np.array_equal((n + 16384).astype(np.int32).astype(np.int64), n + 16384)
    assert R.sharpen(vs, hi, t, w, h, strength=32)[3, 3].tolist() == [65535] * 3 and R.sharpen(vs, lo, t, w, h, strength=32)[3, 3].tolist() == [0] * 3
    assert R.sharpen(vs, hi, t, w, h, strength=32)[3, 4].tolist() == [0] * 3      # (a neighbour: 0 - 256 * 65535 * 32 / 32768 clamps at 0)


def test_hand_computed_3x3(vs):
    """the window (2, 2, 3, 3) of an 8 x 8 frame under the shift (-1/2, -1/4): a = 16, b = 8, va = 256, vb = 192"""
    t = vs.Transform.of(0, 0, -0.5, -0.25)
    X, Y = R.positions(vs, t, 8, 8)
    assert X[3, 3] == 32 * 3 + 16 and Y[3, 3] == 32 * 3 + 8
    win = np.zeros((3, 3, 3), np.uint8)
    #            c              l              r              u              d
    win[1, 1], win[1, 0], win[1, 2], win[0, 1], win[2, 1] = (100, 200, 250), (90, 100, 0), (120, 100, 0), (80, 200, 0), (130, 200, 0)
    # ch 0: 16 (256 (200 - 210) + 192 (200 - 210)) = -71680; (-71680 + 16384) >> 15 = -2
    # ch 1: 16 (256 (400 - 200) + 192 * 0) = 819200; (819200 + 16384) >> 15 = 25
    # ch 2: 16 (256 * 500 + 192 * 500) = 3584000; (3584000 + 16384) >> 15 = 109; 250 + 109 clamps at 255
    assert R.numerators(vs, win, t, 8, 8, roi=(2, 2, 3, 3))[1, 1].tolist() == [-71680, 819200, 3584000]
    out = R.sharpen(vs, win, t, 8, 8, roi=(2, 2, 3, 3))
    assert out[1, 1].tolist() == [98, 225, 255]
    ring = np.ones((3, 3), bool)
    ring[1, 1] = False
    assert np.array_equal(out[ring], win[ring])
    # at the frame's right edge the centre's right neighbour is not covered: nothing changes
    assert np.array_equal(R.sharpen(vs, win, t, 8, 8, roi=(5, 2, 3, 3)), win)


@pytest.mark.parametrize("dtype,maxv", FORMATS)
def test_restatement_equals_the_float64_form(vs, dtype, maxv):
    T = vs.Transform.of
    rng = np.random.default_rng(7 + maxv)
    w, h = 45, 31
    for t in (T(0.03, 0.05, 1.3, -0.7), T(0, 0, 0.5, 0.5), T(-0.1, 0.2, 6.25, 4.0), T(0, 0, 0.03125, 0.96875)):
        img = _noise(rng, h, w, dtype, 65535 if dtype == np.uint16 else 255)     # (16-bit containers: samples above the maximum too)
        for s in (1, 16, 32):
            for roi in (None, (3, 2, 30, 20)):
                win = img if roi is None else img[roi[1]:roi[1] + roi[3], roi[0]:roi[0] + roi[2]]
                a, b = R.sharpen(vs, win, t, w, h, roi, s, maxv), R.sharpen_float(vs, win, t, w, h, roi, s, maxv)
                assert np.array_equal(a, b) and (a != win).any()


def test_defaults_symbols_and_argument_checks(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_sharpen_params_default", "vs_bgr_sharpen_batch", "vs_stabilizer_set_sharpen", "vs_stabilizer_get_sharpen"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
    assert vs.sharpen_params().strength == 16
    ident = vs.Transform.of()
    src = np.full((2, 4, 6, 3), 100, np.uint8)
    # every refusal comes before any device work: VS_ERR_ARG (-1) with or without a device; an accepted call gets as far as the device (-2 where
    # there is none)
    for s, ok in ((0, False), (1, True), (16, True), (32, True), (33, False), (-1, False)):
        if ok:
            try:
                vs.sharpen_batch(src, [ident, ident], 6, 4, params=vs.sharpen_params(strength=s))
            except vs.VsError as e:
                assert "error -2" in str(e), e
        else:
            with pytest.raises(vs.VsError, match="error -1"):
                vs.sharpen_batch(src, [ident, ident], 6, 4, params=vs.sharpen_params(strength=s))
    lib = vs.lib()
    t2 = (vs.Transform * 2)(ident, ident)
    dst = np.zeros_like(src)
    sp, dp = src.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p)

    def call(src_p=sp, fs=72, n=2, w=6, h=4, fmt=vs.FMT_BGR8, t_p=t2, rx=0, ry=0, rw=6, rh=4, ss=18, dst_p=dp, dfs=72, ds=18, mem=vs.MEM_HOST):
        return lib.vs_bgr_sharpen_batch(src_p, fs, n, w, h, fmt, t_p, None, rx, ry, rw, rh, ss, dst_p, dfs, ds, mem, None)
    for kw in (dict(src_p=None), dict(dst_p=None), dict(t_p=None), dict(n=-1), dict(w=0), dict(h=-1), dict(ss=17), dict(ds=17), dict(fs=71), dict(dfs=71),
               dict(fmt=vs.FMT_GRAY8), dict(fmt=99), dict(mem=7),
               # a window outside the frame
               dict(rx=1), dict(ry=1), dict(rx=-1, rw=5), dict(rw=7), dict(rh=5), dict(rw=0), dict(rh=0),
               # the stencil cannot run in place: the same buffer, and ranges that overlap by one row
               dict(dst_p=sp), dict(dst_p=ctypes.c_void_p(sp.value + 18)), dict(src_p=ctypes.c_void_p(dp.value + 2 * 72 - 1))):
        assert call(**kw) == -1, kw
    assert call(n=0) == 0                                                # nothing to do is no error, with or without a device
    assert call(n=0, src_p=None, dst_p=None, t_p=None) == 0
    assert call(n=0, rw=7) == -1                                         # ... but the window is still checked
    assert call(w=32768, h=4) == -3 and call(w=6, h=32768) == -3         # VS_ERR_UNSUPPORTED, as the fill
    sp1 = vs.SharpenParams(0)
    assert lib.vs_bgr_sharpen_batch(sp, 72, 2, 6, 4, vs.FMT_BGR8, t2, ctypes.byref(sp1), 0, 0, 6, 4, 18, dp, 72, 18, vs.MEM_HOST, None) == -1
    for fn, args in ((lib.vs_stabilizer_set_sharpen, (None, None)), (lib.vs_stabilizer_get_sharpen, (None, None))):
        assert fn(*args) == -1


PHASES = ((4, 4), (16, 0), (16, 16))


@pytest.mark.parametrize("cut", (0.15, 0.25))
def test_premise_directions(oracle, cut):
    """DESIGN.md section 28's table, rebuilt: only directions are asserted, the values are printed (pytest -s) and stand in the document"""
    zero = R.premise_case(oracle, cut, 0, 0)
    assert zero[16] == zero[0] and abs(zero[0][1] - 1.0) < 0.01          # phase 0: unchanged, and the warp is the rounded texture itself
    plain, sharp = [zero[0][1]], [zero[16][1]]
    for a, b in PHASES:
        res = R.premise_case(oracle, cut, a, b, strengths=(16, 24))
        print("cut %.2f phase (%2d, %2d): plain %.1f dB ge %.2f | strength 16: %.1f dB ge %.2f | strength 24: %.1f dB ge %.2f"
              % (cut, a, b, *res[0], *res[16], *res[24]))
        assert res[16][0] > res[0][0], (cut, a, b, res)                  # closer to the true shift than the plain warp
        plain.append(res[0][1])
        sharp.append(res[16][1])
    # the gradient energy pulses less from phase to phase: over the non-zero phases, and over all of them (phase 0 has ge 1)
    assert max(sharp[1:]) - min(sharp[1:]) < max(plain[1:]) - min(plain[1:]), (cut, plain, sharp)
    assert max(sharp) - min(sharp) < max(plain) - min(plain), (cut, plain, sharp)
