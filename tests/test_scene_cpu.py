"""-m "not gpu": the scene-cut rule's restatement (tests/_scene_ref.py) checked for the rule's exact consequences, the host decision
(vs_scene_cuts) at its boundaries and against the restatement, the defaults, the argument checks, the new public symbols, and the premise of
the engine tests: on the synthetic clips they use, frames of one scene stay under the threshold and frames of different scenes above it.

Nothing here needs a device: the statistics come from the restatement, the decision is host code."""
import ctypes

import numpy as np
import pytest

import _scene_ref as R

FORMATS = ((np.uint8, 8), (np.uint16, 10), (np.uint16, 16))


@pytest.mark.parametrize("dtype,bits", FORMATS)
def test_the_three_consequences(vs, dtype, bits):
    T = vs.Transform.of
    rng = np.random.default_rng(bits)
    h, w, step = 30, 44, 2
    maxv = (1 << bits) - 1
    a = rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)
    L = R.lattice_size(w, h, step)
    assert L == 15 * 22
    # (a) identical frames under the identity
    assert R.pair_stats(vs, a, a, T(), bits, step) == [L, 0]
    # (b) a copy shifted by whole pixels, under that shift: target (x, y) is the candidate's pixel (x - 3, y - 2)
    b = rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)
    b[:h - 2, :w - 3] = a[2:, 3:]
    t = T(0, 0, 3, 2)
    M = vs.cv_inverse_matrix(t, w, h)
    assert (M[2], M[5]) == (-3.0, -2.0)
    overlap = len(range(4, w, step)) * len(range(2, h, step))           # lattice pixels with x >= 3 and y >= 2
    assert R.pair_stats(vs, a, b, t, bits, step) == [overlap, 0]
    assert R.pair_stats(vs, a, b, T(), bits, step)[1] > 0               # ... and not under the identity
    # (c) constant frames of 100 and 130, at the format's scale
    lo, hi = np.full((h, w, 3), 100 << (bits - 8), dtype), np.full((h, w, 3), 130 << (bits - 8), dtype)
    assert R.pair_stats(vs, lo, hi, T(), bits, step) == [L, 90 * L]
    assert R.pair_stats(vs, hi, lo, T(), bits, step) == [L, 90 * L]
    # samples above the format's maximum are the maximum; black and clipped samples count
    if bits == 10:
        over = np.full((h, w, 3), 65535, dtype)
        assert R.pair_stats(vs, over, np.full((h, w, 3), 1023, dtype), T(), bits, step) == [L, 0]
    assert R.pair_stats(vs, np.zeros((h, w, 3), dtype), np.full((h, w, 3), maxv, dtype), T(), bits, step) == [L, 3 * 255 * L]
    # a map that is not finite counts nothing
    assert R.pair_stats(vs, a, a, T(float("nan"), 0, 0, 0), bits, step) == [0, 0]


def test_decision_boundaries(vs):
    """at 2^30-scale counts, so that a 32-bit product or comparison shows"""
    w, h = 65535, 65535
    for step, thr in ((1, 32), (1, 255), (4, 2), (64, 200)):
        need = R.min_count(w, h, step)
        count = 2 ** 30 - 1
        assert count >= need and 3 * thr * count > 2 ** 32
        rows = [[count, 3 * thr * count], [count, 3 * thr * count + 1], [count, 0], [need, 0], [need - 1, 0], [0, 0], [need, 3 * thr * need], [need, 3 * thr * need + 1]]
        want = [0, 1, 0, 0, 1, 1, 0, 1]
        assert R.cuts(rows, w, h, step, thr).tolist() == want
        assert vs.scene_cuts(np.array(rows, np.uint64), w, h, vs.scene_params(step=step, threshold=thr)).tolist() == want
    # the largest lattice: L / 16 = 2^28 - ..., one below is a cut whatever sad is
    need = R.min_count(65535, 65535, 1)
    assert need == (65535 * 65535) // 16 > 2 ** 27
    assert vs.scene_cuts(np.array([[need - 1, 0], [need, 0]], np.uint64), 65535, 65535, vs.scene_params(step=1)).tolist() == [1, 0]
    # a lattice of fewer than 16 pixels: one pair is enough, none is a cut
    assert R.min_count(12, 9, 4) == 1
    assert vs.scene_cuts(np.array([[1, 96], [1, 97], [0, 0]], np.uint64), 12, 9).tolist() == [0, 1, 1]


def test_decision_against_the_restatement(vs):
    rng = np.random.default_rng(27)
    for w, h, step, thr in ((160, 128, 4, 32), (64, 48, 1, 5), (1920, 1080, 3, 255), (7, 5, 64, 1)):
        need = R.min_count(w, h, step)
        count = rng.integers(0, 4 * need + 2, 400).astype(np.uint64)
        sad = (count.astype(np.float64) * 3 * thr * rng.uniform(0.0, 2.0, 400)).astype(np.uint64)
        sad[::7] = 3 * thr * count[::7]                                  # equality now and then
        stats = np.stack([count, sad], axis=1)
        got = vs.scene_cuts(stats, w, h, vs.scene_params(step=step, threshold=thr))
        assert np.array_equal(got, R.cuts(stats, w, h, step, thr))
        assert 0 < got.sum() < 400
    assert vs.scene_cuts(np.zeros((0, 2), np.uint64), 16, 16).size == 0


def test_defaults_symbols_and_argument_checks(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_scene_params_default", "vs_bgr_scene_stats_batch", "vs_scene_cuts", "vs_stabilizer_set_scene_cut", "vs_stabilizer_get_scene_cut",
                 "vs_stabilizer_get_scene_cuts"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
    p = vs.scene_params()
    assert (p.step, p.threshold) == (4, 32)
    # every refusal comes before any device work: VS_ERR_ARG (-1) with or without a device; an accepted call gets as far as the device (-2 where
    # there is none)
    src = np.full((2, 4, 4, 3), 100, np.uint8)
    ident = vs.Transform.of()
    stats = np.zeros((1, 2), np.uint64)
    for kw, ok in ((dict(step=0), False), (dict(step=1), True), (dict(step=64), True), (dict(step=65), False), (dict(threshold=0), False),
                   (dict(threshold=1), True), (dict(threshold=255), True), (dict(threshold=256), False), (dict(step=-1), False)):
        q = vs.scene_params(**kw)
        if ok:
            assert vs.scene_cuts(stats, 4, 4, q).tolist() == [1]
            try:
                vs.scene_stats_batch(src, [[0, 1]], [ident], params=q)
            except vs.VsError as e:
                assert "error -2" in str(e), e
        else:
            with pytest.raises(vs.VsError, match="error -1"):
                vs.scene_cuts(stats, 4, 4, q)
            with pytest.raises(vs.VsError, match="error -1"):
                vs.scene_stats_batch(src, [[0, 1]], [ident], params=q)
    # a frame index out of range, on either side of a pair
    for pair in ([0, 2], [2, 0], [-1, 0], [0, -1]):
        with pytest.raises(vs.VsError, match="error -1"):
            vs.scene_stats_batch(src, [pair], [ident])
    # negative counts, NULLs, sizes
    lib = vs.lib()
    idx = (ctypes.c_int32 * 2)(0, 1)
    t1 = (vs.Transform * 1)(ident)
    out = np.zeros(2, np.uint64)
    sp, op = src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)

    def stats_call(src_p=sp, n_src=2, w=4, h=4, stride=12, fmt=vs.FMT_BGR8, n_pairs=1, idx_p=idx, t_p=t1, out_p=op):
        return lib.vs_bgr_scene_stats_batch(src_p, 48, n_src, w, h, stride, fmt, n_pairs, idx_p, t_p, None, out_p, vs.MEM_HOST, None)
    for kw in (dict(src_p=None), dict(idx_p=None), dict(t_p=None), dict(out_p=None), dict(n_pairs=-1), dict(n_src=0), dict(n_src=-3), dict(w=0), dict(h=-1),
               dict(stride=11), dict(fmt=vs.FMT_GRAY8)):
        assert stats_call(**kw) == -1, kw
    assert stats_call(n_pairs=0) == 0                                    # nothing to do is no error, with or without a device
    assert stats_call(n_pairs=0, idx_p=None, t_p=None, out_p=None) == 0
    big = np.zeros((1, 1, 32768, 3), np.uint8)
    with pytest.raises(vs.VsError, match="error -3"):
        vs.scene_stats_batch(big, [[0, 0]], [ident])
    cut = np.zeros(1, np.uint8)
    cp, stp = cut.ctypes.data_as(ctypes.c_void_p), stats.ctypes.data_as(ctypes.c_void_p)
    assert lib.vs_scene_cuts(stp, 1, 4, 4, None, cp) == 0
    for args in ((None, 1, 4, 4, None, cp), (stp, 1, 4, 4, None, None), (stp, -1, 4, 4, None, cp), (stp, 1, 0, 4, None, cp), (stp, 1, 4, -2, None, cp)):
        assert lib.vs_scene_cuts(*args) == -1, args
    for fn, args in ((lib.vs_stabilizer_set_scene_cut, (None, None)), (lib.vs_stabilizer_get_scene_cut, (None, None)),
                     (lib.vs_stabilizer_get_scene_cuts, (None, None, 0))):
        assert fn(*args) == -1


SEEDS_B = (4, 5, 7, 11, 19, 23, 42)


@pytest.fixture(scope="module")
def clips():
    """per (size, seed): the 12-frame BGR clip of the engine tests and its path (made once, left unchanged)"""
    from video_stabilizer_amd import synth
    cache = {}

    def get(w, h, seed):
        if (w, h, seed) not in cache:
            cache[(w, h, seed)] = synth.make_clip(w, h, 12, seed=seed, channels=3, pan=4.0, jitter_t=6.0)
        return cache[(w, h, seed)]
    return get


@pytest.mark.parametrize("w,h", ((160, 128), (64, 48)))
def test_premise_of_the_engine_tests(vs, clips, w, h):
    """The clips of tests/test_scene_stab_gpu.py: within scene 3, under the path's true translation standing in for the aligner's measurement,
    the mean absolute difference stays under the default threshold; a cut from scene 3 to each of seven other scenes stays above it, under the
    same kind of motion and under the identity.  Expected (include/vs_amd.h): about 1.2 levels against at least 48."""
    T = vs.Transform.of
    p = vs.scene_params()
    a, path = clips(w, h, 3)

    def motion(p0, p1):                                                  # frame j-1 samples the scene at +p0, frame j at +p1: the content moves by p0 - p1
        return R.pair_transform(vs, T(0, 0, p0[2] - p1[2], p0[3] - p1[3]))
    within = [R.pair_stats(vs, a[j - 1], a[j], motion(path[j - 1], path[j]), 8, p.step) for j in range(1, len(a))]
    assert all(row[0] >= R.min_count(w, h, p.step) for row in within)
    worst = max(R.mean_level(row) for row in within)
    still = max(R.mean_level(R.pair_stats(vs, a[j - 1], a[j], T(), 8, p.step)) for j in range(1, len(a)))
    across = []
    for seed in SEEDS_B:
        b, pb = clips(w, h, seed)
        across.append(R.mean_level(R.pair_stats(vs, a[-1], b[0], motion(path[-1], pb[0]), 8, p.step)))
        across.append(R.mean_level(R.pair_stats(vs, a[-1], b[0], T(), 8, p.step)))
    print("%d x %d: within a scene max %.2f (identity motion: %.2f), cuts min %.1f max %.1f" % (w, h, worst, still, min(across), max(across)))
    assert worst < p.threshold < min(across)
    assert worst < 3.0 and min(across) > 40.0                            # the table's figures, with room: 1.2 and 48
    assert not R.cuts(np.array(within, np.uint64), w, h, p.step, p.threshold).any()
