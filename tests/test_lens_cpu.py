"""The lens map and the remap on the CPU: vs_lens_map in host memory (no device needed) against the rule's numpy restatement
(tests/_lens_ref.py), bit for bit; the remap's restatement against the oracle's VS_WARP_BILINEAR_CV warp and the rule's consequences (a) - (c);
the direction test against frames rendered through the forward lens model."""
import numpy as np
import pytest

import _fill_ref as FR
import _lens_ref as L

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
SIZES = [(1, 1), (2, 3), (96, 64), (1920, 8)]
# a plain radial-tangential lens, a strong barrel, a rational one, one whose denominator 1 + k4 r2 passes through 0 inside the frame (r2 reaches
# 0.2 well inside a frame whose r2 goes to 0.36 and beyond), and a zoomed camera with an off-centre principal point
COEFFS = {"brown": dict(k1=-0.25, k2=0.05, p1=0.001, p2=-0.002), "barrel": dict(k1=-0.4, k2=0.12, k3=-0.02),
          "rational": dict(k1=-0.3, k2=0.1, p1=0.0005, p2=0.0005, k3=-0.01, k4=0.01, k5=0.02, k6=-0.003),
          "pole": dict(k1=0.1, k4=-5.0), "zoomed": dict(k1=0.2, zoom=1.3, cx=10.25, cy=-3.5, fx=77.7, fy=80.1)}


def _both(vs, w, h, **kw):
    return vs.lens_params(w, h, **kw), L.params(w, h, **kw)


@pytest.mark.parametrize("name", sorted(COEFFS))
def test_the_host_map_equals_the_rule(vs, name):
    for w, h in SIZES:
        pv, pl = _both(vs, w, h, **COEFFS[name])
        assert pv.tup()[:13] == tuple(float(pl[k]) for k in L.FIELDS)        # the defaults agree too
        want = L.lens_map(pl, w, h)
        got = vs.lens_map(pv, w, h)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, w, h, int((got != want).sum()))
        # a pitched map between guard rows: the padding and the rows around the map stay untouched
        ms = 2 * w + 5
        res, buf = vs.lens_map(pv, w, h, map_stride=ms, guard=0x5A5A5A5A)
        assert np.array_equal(res, want)
        assert (buf[:2] == 0x5A5A5A5A).all() and (buf[h + 2:] == 0x5A5A5A5A).all() and (buf[2:h + 2, 2 * w:] == 0x5A5A5A5A).all()
    if name == "pole":                                               # the premise: the denominator changes sign inside the 96 x 64 frame
        p = L.params(96, 64, **COEFFS[name])
        u, v = np.meshgrid(np.arange(96.0), np.arange(64.0))
        den = 1 + p["k4"] * (((u - p["cx"]) / p["fx"]) ** 2 + ((v - p["cy"]) / p["fy"]) ** 2)
        assert den.min() < 0 < den.max()


def test_a_denominator_of_exactly_zero_is_defined_by_the_rounding(vs):
    """fx = fy = 1 about (0, 0) with k4 = -1: at r2 == 1 the denominator is exactly 0, kr is an infinity (or, 0 / 0 with k1 = -1, a NaN):
    the position saturates, or is 0"""
    w, h = 4, 3
    for k1 in (0.0, -1.0):
        kw = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, k1=k1, k4=-1.0)
        pv, pl = _both(vs, w, h, **kw)
        want = L.lens_map(pl, w, h)
        got = vs.lens_map(pv, w, h)
        assert np.array_equal(got, want)
        assert tuple(got[0, 1]) == ((INT_MAX, 0) if k1 == 0.0 else (0, 0))       # (u, v) = (1, 0): x * inf, y * inf = 0 * inf = NaN -> 0
        assert tuple(got[0, 0]) == (0, 0)


def test_the_identity_lens_gives_32u_32v(vs):
    for w, h in ((1920, 3), (7, 1080), (96, 64)):
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        want = np.stack([32 * u, 32 * v], axis=2)
        assert np.array_equal(vs.lens_map(vs.lens_params(w, h), w, h), want)
        for f in (0.1, 1.0, 3.7, 517.3, 3000.0):
            pv, pl = _both(vs, w, h, fx=f, fy=f * 1.01, cx=w / 3.0, cy=h * 0.7)
            assert np.array_equal(vs.lens_map(pv, w, h), want), (w, h, f)
            assert np.array_equal(L.lens_map(pl, w, h), want), (w, h, f)


def test_the_map_s_argument_errors(vs):
    w, h = 8, 6
    assert vs.lens_map(vs.lens_params(w, h, k1=0.1), w, h).shape == (h, w, 2)
    bad = [dict(k1=float("nan")), dict(k6=float("inf")), dict(cx=float("-inf")), dict(fx=0.0), dict(fy=-1.0), dict(zoom=0.0), dict(zoom=-2.0),
           dict(zoom=float("nan")), dict(fx=float("inf"))]
    for kw in bad:
        with pytest.raises(vs.VsError, match="error -1"):
            vs.lens_map(vs.lens_params(w, h, **kw), w, h)
    with pytest.raises(vs.VsError, match="error -1"):               # a row does not hold its pairs
        vs.lens_map(vs.lens_params(w, h), w, h, map_stride=2 * w - 1)
    buf = np.zeros((4, 4), np.int32)
    p = vs.lens_params(2, 2)
    for ww, hh in ((0, 2), (2, 0), (32768, 1), (1, 32768)):
        assert vs.lib().vs_lens_map(vs.C.byref(p), ww, hh, buf.ctypes.data_as(vs.C.c_void_p), 65536, vs.MEM_HOST, None) == -1
    assert vs.lib().vs_lens_map(None, 2, 2, buf.ctypes.data_as(vs.C.c_void_p), 4, vs.MEM_HOST, None) == -1
    assert vs.lib().vs_lens_map(vs.C.byref(p), 2, 2, None, 4, vs.MEM_HOST, None) == -1
    assert vs.lib().vs_lens_map(vs.C.byref(p), 2, 2, buf.ctypes.data_as(vs.C.c_void_p), 4, 7, None) == -1      # no such memory


# ---- the remap's restatement ----------------------------------------------------------------------------------------------------------------
MOTIONS = [(0.0, 0.0, 7.0, -3.0), (0.02, -0.03, 2.5, 1.25), (-0.01, 0.015, -4.0, 6.5), (0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.5, -1.5)]


def _noise(rng, w, h, dtype, maxv):
    return rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)


def _warp_positions(O, t, w, h):
    """VS_WARP_BILINEAR_CV's own positions of every pixel: (h, w, 2)"""
    X0, Y0, ad, bd = FR._table_terms(O, t, w, h, FR.cv_round_sat)
    return np.stack([FR.wrap32(FR.wrap32(X0 + 16) + ad) >> 5, FR.wrap32(FR.wrap32(Y0 + 16) + bd) >> 5], axis=2)


@pytest.mark.parametrize("dtype,maxv", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_the_remap_restatement_is_the_oracle_s_warp_where_the_taps_are_inside(oracle, dtype, maxv):
    O = oracle
    rng = np.random.default_rng(maxv)
    w, h = 61, 37
    frame = _noise(rng, w, h, dtype, maxv)
    seen = 0
    for tup in MOTIONS:
        t = O.Transform.of(*tup)
        pos = _warp_positions(O, t, w, h)
        cov = L.taps_inside(pos, w, h)
        assert np.array_equal(cov, FR.covered(O, t, w, h)) and cov.mean() > 0.5
        want = O.bgr_image_warp(frame, t, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=maxv)
        for border in (L.BORDER_CLAMP, L.BORDER_CONSTANT):
            got = L.remap(frame, pos, border, maxv)
            assert np.array_equal(got[cov], want[cov]), (tup, border)
        seen += int(((pos[..., 0] & 31 != 0) | (pos[..., 1] & 31 != 0))[cov].sum())
    assert seen > 1000                                               # the comparison was about interpolated samples


@pytest.mark.parametrize("dtype,maxv", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_the_remap_s_consequences(dtype, maxv):
    rng = np.random.default_rng(3 + maxv)
    for w, h in ((33, 21), (64, 16), (5, 1), (1, 7), (1, 1)):
        frame = _noise(rng, w, h, dtype, maxv)
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        ident = np.stack([32 * u, 32 * v], axis=2)
        # (a) the identity map, under both borders
        for border in (L.BORDER_CLAMP, L.BORDER_CONSTANT):
            assert np.array_equal(L.remap(frame, ident, border, maxv), frame)
        # (b) clamp border: between the frame's extremes per channel, for positions inside, across the edges and far outside, any output size
        dull = (frame // 3 + maxv // 4).astype(dtype)
        pos = rng.integers(-40 * 32, (max(w, h) + 40) * 32, (h + 3, w + 2, 2))
        out = L.remap(dull, pos, L.BORDER_CLAMP, maxv)
        assert out.shape == (h + 3, w + 2, 3)
        for c in range(3):
            assert dull[..., c].min() <= out[..., c].min() and out[..., c].max() <= dull[..., c].max()
        # the constant border differs from the clamp border exactly where a tap is outside, and never exceeds it
        outc = L.remap(dull, pos, L.BORDER_CONSTANT, maxv)
        ins = L.taps_inside(pos, w, h)
        assert np.array_equal(outc[ins], out[ins]) and (outc <= out).all() and (w * h == 1 or (outc[~ins] < out[~ins]).any())
    # (c) every sample is defined for every map: the extremes of int32 land on a corner pixel (clamp) or on 0 (constant), fraction included
    frame = _noise(rng, 9, 7, dtype, maxv)
    frame[0, 0], frame[-1, -1], frame[0, -1], frame[-1, 0] = (1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)
    pos = np.array([[[INT_MIN, INT_MIN], [INT_MAX, INT_MAX], [INT_MAX, INT_MIN], [INT_MIN, INT_MAX]]])
    assert np.array_equal(L.remap(frame, pos, L.BORDER_CLAMP, maxv)[0], [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]])
    assert not L.remap(frame, pos, L.BORDER_CONSTANT, maxv).any()


def test_samples_above_the_format_s_maximum_saturate():
    """a 10-bit container that holds 16-bit values: the identity map saturates them (the blend at zero fraction is the sample), the clamp to the
    format's maximum is the blend's last step"""
    frame = np.full((4, 5, 3), 60000, np.uint16)
    u, v = np.meshgrid(np.arange(5), np.arange(4))
    assert (L.remap(frame, np.stack([32 * u, 32 * v], axis=2), L.BORDER_CLAMP, 1023) == 1023).all()


# ---- direction --------------------------------------------------------------------------------------------------------------------------------
def test_direction_on_the_restatement():
    """the corrected frame is close to what an ideal camera sees, and the correction with every coefficient negated is further from it than the
    raw frame: the map runs from the ideal frame into the distorted one, not the other way.  The thresholds, 0.1 and 1.1, sit over this
    restatement's own figures (DESIGN.md "Lens-distortion correction"): corrected 0.015 .. 0.026 of raw, negated 1.18 .. 1.86 of raw."""
    errs = L.direction_errors(lambda f, p: L.remap(f, L.lens_map(p, f.shape[1], f.shape[0]), L.BORDER_CLAMP, 255))
    for raw, right, wrong in errs:
        print("raw %.3f  corrected %.3f (%.3f)  negated %.3f (%.2f)" % (raw, right, right / raw, wrong, wrong / raw))
    for raw, right, wrong in errs:
        assert raw > 5.0                                             # the lens did distort the frame
        assert right <= 0.1 * raw
        assert wrong >= 1.1 * raw
