"""-m "not gpu": the dense-flow specification (tests/_flow_ref.py) on known answers, and the flow ABI without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_cases as K  # noqa: E402
import _flow_direct as D  # noqa: E402
import _flow_ref as R  # noqa: E402
from _flow_cases import band_limited  # noqa: E402,F401  (test_flow_gpu.py takes it from here)


def shifted_pair(h, w, dx, dy, seed=1, margin=20):
    """(prev, next) u8 with next(x, y) = prev(x - dx, y - dy): the true flow is (dx, dy) everywhere"""
    t = band_limited(h + 2 * margin, w + 2 * margin, seed)
    a = t[margin:margin + h, margin:margin + w]
    b = t[margin - dy:margin - dy + h, margin - dx:margin - dx + w]
    return np.clip(a, 0, 255).round().astype(np.uint8), np.clip(b, 0, 255).round().astype(np.uint8)


@pytest.mark.parametrize("poly_n,poly_sigma", [(5, 1.2), (7, 1.5), (3, 0.9)])
def test_polynomial_expansion_recovers_a_quadratic(poly_n, poly_sigma):
    h, w = 48, 56
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    c = (3.0, 0.5, -0.25, 0.01, 0.02, -0.015)           # 1, x, y, x^2, y^2, xy
    f = c[0] + c[1] * x + c[2] * y + c[3] * x * x + c[4] * y * y + c[5] * x * y
    E = R.poly_exp(f.astype(np.float32), poly_n, poly_sigma)
    sl = (slice(poly_n, h - poly_n), slice(poly_n, w - poly_n))
    yy, xx = y[sl], x[sl]
    want = [c[1] + 2 * c[3] * xx + c[5] * yy, c[2] + 2 * c[4] * yy + c[5] * xx, np.full_like(xx, c[3]), np.full_like(xx, c[4]),
            np.full_like(xx, c[5] / 2)]
    for k in range(5):
        np.testing.assert_allclose(E[k][sl], want[k], rtol=0, atol=2e-4 * max(1.0, np.abs(want[k]).max()), err_msg="coefficient %d" % k)


def test_identical_frames_give_zero_flow():
    a, _ = shifted_pair(90, 120, 0, 0, seed=4)
    fl = R.dense_flow(a, a)
    assert fl.shape == (90, 120, 2) and fl.dtype == np.float32
    assert np.all(fl == 0)
    assert R.pair_median(fl) == 0


@pytest.mark.parametrize("dx,dy", [(1, 0), (0, -1), (3, -2), (6, 6), (-6, 4), (-5, -6), (2, 5)])
def test_integer_shift_recovered(dx, dy):
    a, b = shifted_pair(160, 200, dx, dy, seed=2)
    fl = R.dense_flow(a, b)
    inner = fl[30:-30, 30:-30]
    assert abs(float(np.median(inner[..., 0])) - dx) < 0.05
    assert abs(float(np.median(inner[..., 1])) - dy) < 0.05


def test_level_geometry_and_statistic():
    geo = R.level_geometry(97, 61, 0.5, 5)
    assert [g[:2] for g in geo] == [(97, 61), (49, 31), (24, 15), (12, 8), (6, 4), (3, 2)]
    assert R.median_of_pairs([3.0, 1.0, 2.0]) == 2.0
    assert R.median_of_pairs([4.0, 1.0, 2.0, 3.0]) == 2.5
    fl = np.zeros((3, 3, 2), np.float32)
    fl[..., 0] = np.arange(9, dtype=np.float32).reshape(3, 3)
    assert R.pair_median(fl) == 4.0


def test_flow_params_default_through_ctypes(vs):
    p = vs.flow_params()
    assert p.tup() == (0.5, 3, 15, 3, 5, 1.2, 0)
    q = vs.flow_params(levels=5, winsize=21)
    assert (q.levels, q.winsize, q.poly_n) == (5, 21, 5)


def test_dense_flow_without_device(vs):
    if vs.device_count() > 0:
        pytest.skip("a HIP device is present")
    a = np.zeros((16, 16), np.uint8)
    with pytest.raises(vs.VsError, match="no usable HIP device"):
        vs.dense_flow(a, a)
    with pytest.raises(vs.VsError, match="no usable HIP device"):
        vs.flow_jitter(np.zeros((3, 16, 16, 3), np.uint8))


# ---- what the specification does with the hostile inputs of tests/_flow_cases.py (their GPU tests: test_flow_hostile_gpu.py) --------
@pytest.mark.parametrize("name", list(K.CONTENT))
def test_hostile_content_has_the_property_it_is_there_for(name):
    a, b, kw, expect = K.content(name)
    assert a.shape == (K.H, K.W) and a.dtype == np.uint8 and b.dtype == np.uint8
    K.check_content(name, R.dense_flow(a, b, **kw), kw, expect)


def test_tie_cuts_put_element_n_half_inside_and_just_past_a_run_of_zeros():
    far_below, just_below, just_above, far_above = K.tie_cuts()
    half = (K.W * K.H) // 2
    assert far_below < just_below < just_above < far_above and just_above == just_below + 1
    for cut, inside in ((far_below, False), (just_below, False), (just_above, True), (far_above, True)):
        fl = R.dense_flow(*K.tie_pair(cut))
        zeros = int(np.count_nonzero(K.mag2(fl) == 0))
        assert zeros > 1000
        assert (zeros > half) == inside and (R.pair_median(fl) == 0) == inside, (cut, zeros, half, R.pair_median(fl))
    for cut in (just_below, just_above):
        assert abs(K.zeros_of(cut) - half) < 200


def test_small_pairs_exist_at_every_tiny_and_tile_edge_shape():
    for w, h in K.TINY_SHAPES + K.EDGE_SHAPES + [(3, 1)]:
        a, b = K.small_pair(w, h, seed=w + 3 * h)
        assert a.shape == b.shape == (h, w)
        for kw in K.PARAM_SETS:
            assert np.isfinite(R.dense_flow(a, b, **dict(kw, levels=3))).all()


# ---- the specification from a second side: tests/_flow_direct.py (float64, direct form, no code shared with _flow_ref.py) ----------
# Bounds: 8 x the largest deviation measured over the stage's cases when this test was written (the measured figure stands next to each
# bound).  The deviation is float32 rounding of the restatement (and its taps rounded to float32); a wrong tap, window offset or
# inverse-Gram constant moves a stage by parts in a hundred.
def _rel(got, want):
    """largest deviation of any plane, relative to that plane's largest magnitude in the direct form"""
    return max(float(np.abs(np.asarray(g, np.float64) - w).max() / np.abs(w).max()) for g, w in zip(got, want))


def _stage_images():
    return {"band": band_limited(61, 97, 7).astype(np.float32),
            "noise": np.random.default_rng(5).integers(0, 256, (61, 97)).astype(np.float32),
            "smaller_than_the_halo": np.random.default_rng(6).integers(0, 256, (3, 5)).astype(np.float32)}


POLY = [(1, 0.5), (5, 1.2), (7, 1.5)]


@pytest.mark.parametrize("poly_n,poly_sigma", POLY)
@pytest.mark.parametrize("content", ["band", "noise", "smaller_than_the_halo"])
def test_polynomial_expansion_equals_the_direct_least_squares_fit(content, poly_n, poly_sigma):
    L = _stage_images()[content]
    dev = _rel(R.poly_exp(L, poly_n, poly_sigma), D.poly_exp(L, poly_n, poly_sigma))
    print("poly_exp %s n=%d: %.3g" % (content, poly_n, dev))
    assert dev <= 6.4e-5                                       # measured: at most 7.9e-6 (band, poly_n 1), whole plane, borders included


@pytest.mark.parametrize("scale", [0.5, 0.25, 0.8])
@pytest.mark.parametrize("content", ["band", "noise", "smaller_than_the_halo"])
def test_pyramid_level_equals_the_direct_2d_gaussian(content, scale):
    img = _stage_images()[content].astype(np.uint8)
    h, w = img.shape
    wk, hk = max(1, int(w * scale + 0.5)), max(1, int(h * scale + 0.5))
    dev = _rel([R.pyramid_level(img, wk, hk, scale)], [D.pyramid_level(img, wk, hk, scale)])
    print("pyramid_level %s scale=%g: %.3g" % (content, scale, dev))
    assert dev <= 2.8e-5                                       # measured: at most 3.5e-6 (noise, scale 0.8)


@pytest.mark.parametrize("winsize", [1, 2, 15, 31])
@pytest.mark.parametrize("shape", [(61, 97), (3, 5)])
def test_window_sum_and_solve_equal_the_direct_2d_sum(shape, winsize):
    # random planes of a well-conditioned system (G11, G22 in [1, 2], |G12| < 0.5): the window's offsets and the solve are under test, not the
    # cancellation in a determinant near 0.  winsize = 2 is the asymmetric window (offsets -1..0)
    rng = np.random.default_rng(11 + winsize)
    M = np.stack([rng.uniform(1, 2, shape), rng.uniform(-0.5, 0.5, shape), rng.uniform(1, 2, shape), rng.standard_normal(shape),
                  rng.standard_normal(shape)]).astype(np.float32)
    dev = _rel(R.blur_solve(M, winsize), D.blur_solve(M, winsize))
    print("blur_solve %r winsize=%d: %.3g" % (shape, winsize, dev))
    assert dev <= 8.9e-6                                       # measured: at most 1.1e-6 (3 x 5, winsize 31)


@pytest.mark.parametrize("poly_n,poly_sigma", POLY)
@pytest.mark.parametrize("content", ["band", "noise", "smaller_than_the_halo"])
def test_update_equals_the_direct_matrix_form(content, poly_n, poly_sigma):
    L = _stage_images()[content]
    h, w = L.shape
    rng = np.random.default_rng(13)
    R0, R1 = R.poly_exp(L, poly_n, poly_sigma), R.poly_exp(np.roll(L, 1, axis=1), poly_n, poly_sigma)
    dx, dy = rng.uniform(-5, 5, (h, w)).astype(np.float32), rng.uniform(-5, 5, (h, w)).astype(np.float32)      # samples inside and clamped
    dev = _rel(R.update(R0, R1, dx, dy), D.update(R0.astype(np.float64), R1.astype(np.float64), dx.astype(np.float64), dy.astype(np.float64)))
    print("update %s n=%d: %.3g" % (content, poly_n, dev))
    assert dev <= 6.4e-5                                       # measured: at most 8.0e-6 (noise, poly_n 1)


@pytest.mark.parametrize("pair", ["shift", "rotation"])
def test_dense_flow_equals_the_direct_form_end_to_end(pair):
    a, b = shifted_pair(160, 200, 3, -2, seed=2) if pair == "shift" else K.moving_pair(200, 160, seed=3)
    direct, det = D.dense_flow(a, b)
    dev = np.abs(R.dense_flow(a, b).astype(np.float64) - direct)[30:-30, 30:-30]          # every interior pixel, none left out
    print("dense_flow %s: max %.3g px, median %.3g px, smallest determinant %.3g" % (pair, dev.max(), np.median(dev), det[30:-30, 30:-30].min()))
    assert det[30:-30, 30:-30].min() > 1.0                     # (measured: 2.4e4, 3.7e4) the comparison never leans on the regulariser 1e-3
    assert dev.max() <= 3.2e-5                                 # measured: 4.0e-6 px (shift), 2.1e-6 px (rotation); medians 3.0e-7, 2.4e-7
