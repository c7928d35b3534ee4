"""-m gpu: dense optical flow (vs_flow.hip) equals its CPU restatement (tests/_flow_ref.py) bit for bit; the per-pair statistic
is selected exactly on the device; chunked clips equal pair-by-pair calls; and the flow score sees motion the similarity
stand-in cannot (the reason the score exists)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402
from _diff import same  # noqa: E402
from _flow_cases import moving_pair, sample  # noqa: E402
from test_flow_cpu import band_limited, shifted_pair  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", [(320, 240), (1920, 1080), (97, 61), (13, 9), (5, 3), (1, 1), (64, 16), (65, 17)])
def test_dense_flow_equals_restatement_shapes(gpu_vs, w, h):
    a, b = moving_pair(w, h, seed=w * 7 + h)
    got = gpu_vs.dense_flow(a, b)
    assert same(got, R.dense_flow(a, b))


def test_dense_flow_pitched_strides(gpu_vs):
    a, b = moving_pair(200, 90, seed=5)
    big_a = np.zeros((90, 237), np.uint8)
    big_b = np.full((90, 237), 77, np.uint8)
    big_a[:, :200], big_b[:, :200] = a, b
    va, vb = big_a[:, :200], big_b[:, :200]           # row stride 237, not the width
    assert va.strides[0] == 237
    assert same(gpu_vs.dense_flow(va, vb), R.dense_flow(a, b))


PARAMS = [dict(levels=0), dict(levels=1), dict(levels=2), dict(levels=4), dict(levels=5),
          dict(winsize=5), dict(winsize=21), dict(poly_n=7, poly_sigma=1.5), dict(iterations=1), dict(iterations=2),
          dict(iterations=5), dict(pyr_scale=0.8, levels=5), dict(pyr_scale=0.8, winsize=21, poly_n=7, poly_sigma=1.5, iterations=4),
          dict(winsize=4), dict(winsize=1, levels=1)]


@pytest.mark.parametrize("kw", PARAMS, ids=[",".join("%s=%s" % i for i in p.items()) for p in PARAMS])
def test_dense_flow_equals_restatement_params(gpu_vs, kw):
    a, b = moving_pair(173, 118, seed=3)
    got = gpu_vs.dense_flow(a, b, gpu_vs.flow_params(**kw))
    assert same(got, R.dense_flow(a, b, **kw))


def test_identical_frames_zero_and_shift_recovered(gpu_vs):
    a, b = shifted_pair(160, 200, 4, -3, seed=9)
    assert np.all(gpu_vs.dense_flow(a, a) == 0)
    fl = gpu_vs.dense_flow(a, b)
    assert abs(float(np.median(fl[30:-30, 30:-30, 0])) - 4) < 0.05 and abs(float(np.median(fl[30:-30, 30:-30, 1])) + 3) < 0.05


def test_unsupported_flags_and_bad_params(gpu_vs):
    with pytest.raises(gpu_vs.VsError, match="flags"):
        gpu_vs.Flow(gpu_vs.flow_params(flags=256))
    with pytest.raises(gpu_vs.VsError, match="out of range"):
        gpu_vs.Flow(gpu_vs.flow_params(winsize=33))
    # every limit of the parameter check, from both sides
    for kw in (dict(pyr_scale=0.0), dict(pyr_scale=1.0), dict(pyr_scale=float("nan")), dict(levels=-1), dict(levels=16), dict(winsize=0), dict(winsize=32),
               dict(iterations=0), dict(iterations=101), dict(poly_n=0), dict(poly_n=8), dict(poly_sigma=0.0), dict(poly_sigma=float("nan"))):
        with pytest.raises(gpu_vs.VsError, match="out of range"):
            gpu_vs.Flow(gpu_vs.flow_params(**kw))
    for kw in (dict(pyr_scale=0.999), dict(levels=0), dict(levels=15), dict(winsize=1), dict(winsize=31), dict(iterations=1), dict(iterations=100),
               dict(poly_n=1), dict(poly_n=7), dict(poly_sigma=1e-3)):
        gpu_vs.Flow(gpu_vs.flow_params(**kw))               # the last value inside each limit makes a handle


def gray_clip(n, w, h, seed):
    """n gray frames of one band-limited texture under a random shake"""
    t = band_limited(h + 64, w + 64, seed)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([np.clip(sample(t, x + 32 + rng.uniform(-4, 4), y + 32 + rng.uniform(-4, 4)), 0, 255).round().astype(np.uint8)
                     for _ in range(n)])


def test_pair_medians_are_exact_elements_of_the_device_field(gpu_vs):
    fr = gray_clip(6, 211, 157, seed=21)
    f = gpu_vs.Flow()
    med, pm = f.jitter(fr)
    assert pm.shape == (5,) and pm.dtype == np.float32
    for i in range(5):
        fl = f.compute(fr[i], fr[i + 1])
        m2 = (fl[..., 0] * fl[..., 0] + fl[..., 1] * fl[..., 1]).ravel()
        n = m2.size
        assert pm[i] == np.sqrt(np.partition(m2, n // 2)[n // 2]), i
        assert pm[i] == R.pair_median(R.dense_flow(fr[i], fr[i + 1])), i
    assert med == R.median_of_pairs(pm)
    med7, pm7 = f.jitter(fr[:5])                          # an even number of pairs (five above)
    assert med7 == R.median_of_pairs(pm7) and same(pm7, pm[:4])


def test_flow_jitter_equals_restatement_bgr(gpu_vs):
    from video_stabilizer_amd import synth
    fr, _ = synth.make_clip(160, 120, 5, seed=3, channels=3)
    med, pm = gpu_vs.flow_jitter(fr)
    rmed, rpm = R.flow_jitter(fr)
    assert same(pm, rpm) and med == rmed


@pytest.mark.parametrize("bits", [8, 10])
def test_chunked_clip_equals_pair_by_pair(gpu_vs, bits):
    # at 1920x1080 a chunk holds about 12 frames (2 GiB of scratch): 15 frames take two chunks sharing one frame
    from video_stabilizer_amd import synth
    n, w, h = 15, 1920, 1080
    fr, _ = synth.make_clip(w, h, n, seed=5 + bits, channels=3, bits=bits, margin=16, jitter_t=3.0)
    f = gpu_vs.Flow()
    med, pm = f.jitter(fr)
    want = []
    for i in range(n - 1):
        fl = f.compute(R.gray(fr[i], bits), R.gray(fr[i + 1], bits))
        m2 = (fl[..., 0] * fl[..., 0] + fl[..., 1] * fl[..., 1]).ravel()
        want.append(np.sqrt(np.partition(m2, m2.size // 2)[m2.size // 2]))
    assert same(pm, np.array(want, np.float32))
    assert med == R.median_of_pairs(want)


def test_alloc_failures_leave_the_handle_usable(gpu_vs):
    # every allocation of vs_flow_create and of a first vs_flow_jitter fails in turn, as out-of-memory (k > 0, VS_ERR_HIP) and as a
    # throwing host allocation (k < 0, VS_ERR_NOMEM): the call fails cleanly and the same handle then computes the right answer
    vs = gpu_vs
    fr = gray_clip(4, 96, 64, seed=2)
    vs.test_fail_alloc(0)
    want = vs.Flow().jitter(fr)
    vs.test_fail_alloc(0)
    vs.Flow().jitter(fr)
    total = vs.test_fail_alloc(0)
    assert total >= 1
    for sign in (1, -1):
        for k in range(1, total + 3):
            f = None
            vs.test_fail_alloc(sign * k)
            try:
                f = vs.Flow()
                f.jitter(fr)
            except vs.VsError as e:
                assert ("error -2" in str(e)) or ("error -5" in str(e)) or ("failed" in str(e)), str(e)
            vs.test_fail_alloc(0)
            if f is None:
                f = vs.Flow()
            got = f.jitter(fr)
            assert got[0] == want[0] and same(got[1], want[1]), (sign, k)


# ---- independence: what the flow score sees that the similarity stand-in cannot ---------------------------------------------
def similarity_score(vs, frames):
    """apps/jitter.hpp's stand-in: the similarity the library's aligner measures, evaluated on a 33 x 33 lattice"""
    _, ts = vs.Aligner(device=0).align_batch(frames)
    w, h = frames.shape[2], frames.shape[1]
    i = np.arange(33) + 0.5
    u, v = (i * w / 33 - 0.5 * w)[None, :], (i * h / 33 - 0.5 * h)[:, None]
    meds = []
    for t in ts[1:]:
        dx, dy = t.A * u - t.B * v + t.TX, t.B * u + t.A * v + t.TY
        mag = np.sort(np.sqrt(dx * dx + dy * dy).astype(np.float32).ravel())
        meds.append(float(mag[mag.size // 2]))
    return R.median_of_pairs(meds)


def test_flow_score_agrees_with_similarity_on_pure_shake(gpu_vs):
    from video_stabilizer_amd import synth
    fr, _ = synth.make_clip(640, 480, 9, seed=11, channels=3, pan=0.0)
    fl, sim = gpu_vs.flow_jitter(fr)[0], similarity_score(gpu_vs, fr)
    assert sim > 1.0
    assert abs(fl - sim) <= 0.15 * sim, (fl, sim)


def test_flow_score_sees_anisotropic_stretch(gpu_vs):
    s, w, h = 0.02, 640, 480
    t = band_limited(h + 64, w + 64, seed=13)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    plain = np.clip(sample(t, x + 32, y + 32), 0, 255).round()
    # content at q in a plain frame sits at c + diag(1+s, 1-s)(q - c) in a stretched one: flow (s*x, -s*y) about the centre
    stretched = np.clip(sample(t, cx + (x - cx) / (1 + s) + 32, cy + (y - cy) / (1 - s) + 32), 0, 255).round()
    gray = np.stack([plain, stretched, plain, stretched, plain]).astype(np.uint8)
    bgr = np.repeat(gray[..., None], 3, axis=-1)
    analytic = float(np.median(np.hypot(s * (x - cx), s * (y - cy))))
    fl = gpu_vs.flow_jitter(bgr)[0]
    sim = similarity_score(gpu_vs, bgr)
    assert fl >= 0.8 * analytic, (fl, analytic)
    assert sim < 0.2 * analytic, (sim, analytic)
