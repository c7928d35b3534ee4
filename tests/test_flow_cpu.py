"""-m "not gpu": the dense-flow specification (tests/_flow_ref.py) on known answers, and the flow ABI without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402


def band_limited(h, w, seed, cutoff=0.05):
    """seeded white noise low-passed by a Gaussian in frequency (periodic), scaled to about 128 +- 40"""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((h, w))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    t = np.real(np.fft.ifft2(np.fft.fft2(n) * np.exp(-(fx ** 2 + fy ** 2) / (2 * cutoff ** 2))))
    return 128.0 + t / t.std() * 40.0


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
