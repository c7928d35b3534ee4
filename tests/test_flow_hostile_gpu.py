"""-m gpu: the dense flow on inputs chosen to hurt (tests/_flow_cases.py): noise, saturated and constant content, step edges, motion
far beyond the pyramid's reach (flows of thousands of pixels that live on update_px's clamp), results full of subnormal floats and
exact zeros; the device selection asked for an element inside, at the end of and just past a run of thousands of equal values, for
element 0 of one value, for several pairs of one launch that end in different bins; the largest LDS halos on frames smaller than the
halo and on widths around the 64-pixel tile; the 257-tap pyramid blur and the refusal one tap further.  Everything is compared with
tests/_flow_ref.py bit for bit; every case first asserts, on the restatement, the property that makes it hostile."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_cases as K  # noqa: E402
import _flow_ref as R  # noqa: E402
from _diff import same  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- content classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CONTENT))
def test_hostile_content_flow_and_pair_median_equal_restatement(gpu_vs, name):
    a, b, kw, expect = K.content(name)
    want = R.dense_flow(a, b, **kw)
    K.check_content(name, want, kw, expect)
    f = gpu_vs.Flow(gpu_vs.flow_params(**kw))
    assert same(f.compute(a, b), want)
    med, pm = f.jitter(np.stack([a, b]))
    assert pm.shape == (1,) and pm[0] == R.pair_median(want), (pm, R.pair_median(want))
    assert med == float(pm[0])


# ---- ties in the selection -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cuts():
    return K.tie_cuts()


@pytest.mark.parametrize("which", ["far_below", "just_below", "just_above", "far_above"])
def test_selection_inside_and_just_past_a_run_of_equal_values(gpu_vs, cuts, which):
    cut = cuts[["far_below", "just_below", "just_above", "far_above"].index(which)]
    a, b = K.tie_pair(cut)
    want = R.dense_flow(a, b)
    zeros, half = int(np.count_nonzero(K.mag2(want) == 0)), want[..., 0].size // 2
    assert zeros > 1000                                       # a run of equal values, thousands long
    if which.endswith("below"):
        assert zeros <= half and R.pair_median(want) > 0      # element n/2 lies past the run
    else:
        assert zeros > half and R.pair_median(want) == 0      # element n/2 lies inside the run
    if which.startswith("just"):
        assert abs(zeros - half) < 200, (zeros, half)         # ... and the run ends next to it
    f = gpu_vs.Flow()
    assert same(f.compute(a, b), want)
    _, pm = f.jitter(np.stack([a, b]))
    assert pm[0] == R.pair_median(want), (pm, R.pair_median(want), cut)


def test_identical_frames_select_zero(gpu_vs):
    a, _ = K.tie_pair(0)
    med, pm = gpu_vs.Flow().jitter(np.stack([a, a, a]))
    assert med == 0.0 and np.all(pm == 0) and not np.any(np.signbit(pm))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 2), (2, 1), (3, 1)])
def test_selection_on_frames_of_one_to_three_pixels(gpu_vs, w, h):
    # n/2 = 0, 1, 1, 1: element 0 of one value, the larger of two, the middle of three
    a, b = K.small_pair(w, h, seed=w * 5 + h)
    if w * h > 1:
        a = a.copy()
        a.flat[0] ^= 0x40                                     # the pixels of a frame this small are nearly equal: make them differ
    fr = np.stack([a, b, a])
    rmed, rpm = R.flow_jitter(fr)
    med, pm = gpu_vs.Flow().jitter(fr)
    assert same(pm, rpm) and med == rmed
    assert same(gpu_vs.dense_flow(a, b), R.dense_flow(a, b))


@pytest.fixture(scope="module")
def mixed_clip(cuts):
    """six frames, five pairs: all-zero, a tie (element n/2 inside the run of zeros), a scene change, an ordinary pair, all-zero"""
    ta, tb = K.tie_pair(cuts[3])
    ba, bb = K.texture_pair(K.W, K.H, 3, -2, seed=3)
    return np.stack([ta, ta, tb, ba, bb, bb])


@pytest.mark.parametrize("n", [6, 5, 4])
def test_pairs_of_one_launch_end_in_different_bins(gpu_vs, mixed_clip, n):
    fr = mixed_clip[:n]                                       # 5, 4 and 3 pairs: odd and even counts for the clip's median
    rmed, rpm = R.flow_jitter(fr)
    assert rpm[0] == 0 and rpm[1] == 0 and (n < 5 or rpm[3] > 1)
    med, pm = gpu_vs.Flow().jitter(fr)
    assert same(pm, rpm) and med == rmed, (pm, rpm, med, rmed)


# ---- parameters x shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", K.PARAM_SETS, ids=K.ident)
@pytest.mark.parametrize("w,h", K.EDGE_SHAPES)
def test_parameters_on_tile_edge_shapes(gpu_vs, kw, w, h):
    a, b = K.small_pair(w, h, seed=w + 3 * h)
    assert same(gpu_vs.dense_flow(a, b, gpu_vs.flow_params(**kw)), R.dense_flow(a, b, **kw))


@pytest.mark.parametrize("levels", [0, 3])
@pytest.mark.parametrize("kw", K.PARAM_SETS, ids=K.ident)
@pytest.mark.parametrize("w,h", K.TINY_SHAPES)
def test_parameters_on_frames_smaller_than_the_halo(gpu_vs, kw, w, h, levels):
    a, b = K.small_pair(w, h, seed=w + 3 * h)
    kw = dict(kw, levels=levels)                              # levels = 3: the layers collapse to 1 x 1 and stay there
    want = R.dense_flow(a, b, **kw)
    f = gpu_vs.Flow(gpu_vs.flow_params(**kw))
    assert same(f.compute(a, b), want)
    assert f.jitter(np.stack([a, b]))[1][0] == R.pair_median(want)


def test_every_tap_of_the_widest_pyramid_blur(gpu_vs):
    kw = dict(pyr_scale=1.0 / 86, levels=1)
    assert R.pyr_taps(R.level_geometry(K.W, K.H, **kw)[1][2])[1] == 128
    a, b = K.texture_pair(K.W, K.H, 3, -2, seed=3)
    assert same(gpu_vs.dense_flow(a, b, gpu_vs.flow_params(**kw)), R.dense_flow(a, b, **kw))


@pytest.mark.parametrize("kw", [dict(pyr_scale=1.0 / 87, levels=1), dict(pyr_scale=0.1, levels=2)], ids=K.ident)
def test_a_wider_pyramid_blur_is_refused_by_the_call_and_nothing_sticks(gpu_vs, kw):
    vs = gpu_vs
    assert R.pyr_taps(R.level_geometry(K.W, K.H, **kw)[-1][2])[1] > 128
    a, b = K.texture_pair(K.W, K.H, 3, -2, seed=3)
    f = vs.Flow(vs.flow_params(**kw))                         # the parameters are in range: the handle exists
    sentinel = np.float32(-12345.5)
    out = np.full((K.H, K.W, 2), sentinel, np.float32)
    r = vs.lib().vs_flow_compute(f.h, vs._p(a), vs._p(b), K.W, K.H, K.W, vs.MEM_HOST, vs._p(out), 2 * K.W)
    assert r == -3 and b"pyramid blur" in vs.lib().vs_last_error(), (r, vs.lib().vs_last_error())
    assert np.all(out == sentinel)                            # refused on the host: nothing ran, nothing was written
    with pytest.raises(vs.VsError, match="error -3.*pyramid blur"):
        f.jitter(np.stack([a, b]))
    with pytest.raises(vs.VsError, match="error -3.*pyramid blur"):
        f.jitter(np.repeat(np.stack([a, b])[..., None], 3, axis=-1))
    assert same(vs.Flow().compute(a, b), R.dense_flow(a, b))  # no sticky error: a new handle computes the right answer
    assert same(vs.Flow(vs.flow_params(levels=0)).compute(a, b), R.dense_flow(a, b, levels=0))


@pytest.mark.parametrize("pyr_scale", [0.8, 0.95])
def test_sixteen_layers(gpu_vs, pyr_scale):
    kw = dict(pyr_scale=pyr_scale, levels=15)
    a, b = K.texture_pair(K.W, K.H, 3, -2, seed=3)
    assert len(R.level_geometry(K.W, K.H, **kw)) == 16
    assert same(gpu_vs.dense_flow(a, b, gpu_vs.flow_params(**kw)), R.dense_flow(a, b, **kw))
