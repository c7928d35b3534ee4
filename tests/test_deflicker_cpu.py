"""-m "not gpu": the deflicker rule's restatement (tests/_deflicker_ref.py) checked for the rule's exact consequences, for the gains' known
answers and on two quality pins; the parameter boundary and the new public symbols.

Nothing of the GPU code is in the tests but the last: they establish that the reference the GPU tests compare against is the rule, and that
the engine's candidate maps point the right way, before a kernel is involved."""
import ctypes

import numpy as np
import pytest

import _engine_model as EM
import _deflicker_ref as R

FORMATS = ((np.uint8, 8, 255), (np.uint16, 10, 1023), (np.uint16, 12, 4095), (np.uint16, 16, 65535))
UNIT = 32768


def _picture(rng, h, w, dtype, maxv, amp=6):
    """a smooth picture plus noise, every sample well inside the counted levels"""
    scale = (maxv + 1) // 256
    yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
    base = (60 + xx + yy // 2 + 10 * cc) * scale
    return np.clip(base + rng.integers(-amp * scale, amp * scale + 1, (h, w, 3)), scale, 254 * scale).astype(dtype)


@pytest.mark.parametrize("dtype,bits,maxv", FORMATS)
def test_the_five_consequences(oracle, dtype, bits, maxv):
    O = oracle
    T = O.Transform.of
    rng = np.random.default_rng(bits)
    h, w, step = 30, 44, 2
    scale = (maxv + 1) // 256
    a = _picture(rng, h, w, dtype, maxv)
    b = np.minimum(a.astype(np.int64) * 5 // 4, 254 * scale).astype(dtype)
    c = (a.astype(np.int64) * 9 // 8).astype(dtype)
    src = np.stack([a, b, c])
    ident = T()
    L, thr = R.lattice_size(w, h, step), R.threshold(w, h, step)
    assert L == 15 * 22 and thr == L // 16
    # premise: with both neighbours under identity maps every lattice pair counts and the frame does change
    rows = R.stats_frame(O, src, [0, 1, 2], [ident] * 3, bits, step)
    assert rows[0] == [0] * 8 and rows[1][0] == L and rows[2][0] == L
    changed, G = R.deflicker_frame(O, src, [0, 1, 2], [ident] * 3, bits, maxv, step)
    assert G[3] == 2 and not np.array_equal(changed, a)
    # (a) one candidate; a list that ends at once; candidates outside the frame; candidates with fewer than max(1, L / 16) counted pairs
    for cf in ([0], [0, -1, -1], [0, -1, 2]):                           # (a negative index ENDS the list)
        out, G = R.deflicker_frame(O, src, cf, [ident] * len(cf), bits, maxv, step)
        assert np.array_equal(out, a) and G == [UNIT, UNIT, UNIT, 0]
    far = [ident, T(0, 0, 500, 0), T(0, 0, 0, -300)]
    rows = R.stats_frame(O, src, [0, 1, 2], far, bits, step)
    assert rows[1] == [0] * 8 and rows[2] == [0] * 8
    out, G = R.deflicker_frame(O, src, [0, 1, 2], far, bits, maxv, step)
    assert np.array_equal(out, a) and G[3] == 0
    few = T(0, 0, w - 2, 0)                                              # the candidate's two left columns under the target's two right ones: one lattice column
    rows = R.stats_frame(O, src, [0, 1], [ident, few], bits, step)
    assert 0 < rows[1][0] == 15 < thr
    out, G = R.deflicker_frame(O, src, [0, 1], [ident, few], bits, maxv, step)
    assert np.array_equal(out, a) and G == [UNIT, UNIT, UNIT, 0]
    # ... and a frame that comes back does so with its samples above the format's maximum
    if bits in (10, 12):
        over = a.copy()
        over[3, 5] = (65535, maxv + 1, maxv)
        out, _ = R.deflicker_frame(O, np.stack([over, b]), [0, 1], far[:2], bits, maxv, step)
        assert np.array_equal(out, over)
    # (b) identical frames under identity maps
    out, G = R.deflicker_frame(O, np.stack([a, a, a]), [0, 1, 2], [ident] * 3, bits, maxv, step)
    assert np.array_equal(out, a) and G == [UNIT, UNIT, UNIT, 2]
    # (d) the gains' range, any content, any maps
    wild = rng.integers(0, maxv + 1, (4, h, w, 3)).astype(dtype)
    wild[1] = np.minimum(wild[1], 3 * scale)
    wild[2] = np.maximum(wild[2], 250 * scale)
    maps = [ident, T(0.02, -0.05, 1.3, -2.6), T(-0.1, 0.2, -4.2, 3.1), T(0.3, 0.0, 0.5, 0.5)]
    for order in ([0, 1, 2, 3], [1, 2, 0, 3], [2, 1, 3, 0], [3, 0, 1, 2]):
        for st in (1, 2, 5):
            G = R.gains(R.stats_frame(O, wild, order, maps, bits, st), w, h, st)
            assert all(16384 <= g <= 65536 for g in G[:3])
    # (e) the target under an integer shift with every sample halved exactly
    even = (a.astype(np.int64) // 2 * 2 + 2 * scale).astype(dtype)
    half = np.zeros_like(even)
    half[:h - 2, :w - 3] = even[2:, 3:] // 2                             # target (x, y) is the candidate's pixel (x - 3, y - 2)
    rows = R.stats_frame(O, np.stack([even, half]), [0, 1], [ident, T(0, 0, 3, 2)], bits, step)
    assert rows[1][0] >= thr and all(2 * rows[1][4 + ch] == rows[1][1 + ch] for ch in range(3))
    assert all(R.ratio_q15(rows[1][1 + ch], rows[1][4 + ch]) == 16384 for ch in range(3))


@pytest.mark.parametrize("dtype,bits,maxv", FORMATS)
def test_constant_frames_and_the_tie(oracle, dtype, bits, maxv):
    """(c) constant frames of 100 (target) and 200 (one candidate): r = 65536, G = (2 * (32768 + 65536) + 2) / 4 = 49152 and every sample is
    (100 * 49152 + 16384) >> 15 = 150.  The rounded divisions' ties, by hand.  r: a = 65536, b = 65537 is 32768.5 exactly -- the + a makes the
    numerator 65536 * 65538, the division by 131072 is exact and gives 32769: the half goes UP.  a = 256, b = 257 is 32896 exactly:
    (65536 * 257 + 256) / 512 = 32896.5 -> 32896.  G: m = 1 with r = 32769 is 32768.5 -> (2 * 65537 + 2) / 4 = 32769, up again; m = 2 with twice
    32769 is 32768.67 -> (2 * 98306 + 3) / 6 = 32769 by floor of 32769.17."""
    O = oracle
    ident = O.Transform.of()
    h, w = 8, 12
    tgt = np.full((h, w, 3), 100, dtype)
    cand = np.full((h, w, 3), 200, dtype)
    if bits > 8:                                                         # the same levels at the format's scale
        tgt, cand = tgt * (1 << (bits - 8)), cand * (1 << (bits - 8))
    out, G = R.deflicker_frame(O, np.stack([tgt, cand]), [0, 1], [ident, ident], bits, maxv, 1)
    assert G == [49152, 49152, 49152, 1]
    assert (out == 150 * (1 << (bits - 8))).all()
    # the tie of r's division and of G's
    assert R.ratio_q15(65536, 65537) == 32768 + (65536 + 65536) // (2 * 65536) == 32769
    assert (2 * 32768 * 65537 + 65536) % (2 * 65536) == 0               # exactly one half, rounded up by the + a
    assert R.ratio_q15(256, 257) == 32896
    row = [w * h, 65536, 65536, 65536, 65537, 65537, 65537, 0]
    assert R.gains([[0] * 8, row], w, h, 1) == [32769, 32769, 32769, 1]
    assert (2 * (32768 + 2 * 32769) + 3) // 6 == 32769
    assert R.gains([[0] * 8, row, row], w, h, 1) == [32769, 32769, 32769, 2]


def test_gains_known_answers():
    w, h, step = 64, 64, 4
    L, thr = R.lattice_size(w, h, step), R.threshold(w, h, step)
    assert (L, thr) == (256, 16)
    z = [0] * 8
    # m = 0
    assert R.gains([z], w, h, step) == [UNIT, UNIT, UNIT, 0]
    assert R.gains([z, z, z], w, h, step) == [UNIT, UNIT, UNIT, 0]
    # equal sums
    eq = [100, 5000, 6000, 7000, 5000, 6000, 7000, 0]
    assert R.gains([z, eq], w, h, step) == [UNIT, UNIT, UNIT, 1]
    # the clamps at 2 and 1 / 2
    hi = [100, 1000, 1000, 1000, 2000, 2001, 90000, 0]
    assert [R.ratio_q15(hi[1 + c], hi[4 + c]) for c in range(3)] == [65536, 65536, 65536]
    lo = [100, 2000, 2000, 2000, 1000, 999, 1, 0]
    assert [R.ratio_q15(lo[1 + c], lo[4 + c]) for c in range(3)] == [16384, 16384, 16384]
    assert R.ratio_q15(2000, 3999) == (65536 * 3999 + 2000) // 4000 == 65520
    assert R.gains([z, hi], w, h, step) == [49152, 49152, 49152, 1]
    assert R.gains([z, lo], w, h, step) == [24576, 24576, 24576, 1]
    assert R.gains([z, hi, lo, eq], w, h, step) == [(2 * (32768 + 65536 + 16384 + 32768) + 4) // 8] * 3 + [3]
    # count exactly at and one below max(1, L / 16); an unused candidate between used ones does not end anything
    at = [thr] + hi[1:]
    below = [thr - 1] + hi[1:]
    assert R.gains([z, at], w, h, step)[3] == 1 and R.gains([z, below], w, h, step) == [UNIT, UNIT, UNIT, 0]
    assert R.gains([z, below, at], w, h, step) == [49152, 49152, 49152, 1]
    # a lattice of fewer than 16 pixels: one pair is enough
    assert R.threshold(12, 9, 4) == 1 and R.threshold(1, 1, 64) == 1
    assert R.gains([z, [1, 10, 10, 10, 20, 20, 20, 0]], 12, 9, 4) == [49152, 49152, 49152, 1]
    # the sums' bound: every term of the ratio below 2^63
    big = 2 ** 46 - 1
    assert R.ratio_q15(big, big) == UNIT and R.ratio_q15(1, big) == 65536 and R.ratio_q15(big, 1) == 16384
    # the applied sample: saturation, and the unit frame left alone
    f = np.array([[[1023, 600, 1024]]], np.uint16)
    assert R.apply_gain(f, [65536, 49152, 16384], 1023).tolist() == [[[1023, 900, 512]]]
    assert np.array_equal(R.apply_gain(f, [UNIT] * 3, 1023), f)
    assert R.apply_gain(f, [UNIT, UNIT, 32769], 1023).tolist() == [[[1023, 600, 1023]]]


# Quality pin 1 (measured with this restatement, seeds 7 / 11 / 13): std of the successive differences of the log effective gain
# before 0.1110 / 0.1257 / 0.1067, after 0.0272 / 0.0277 / 0.0225, ratio 0.2455 / 0.2201 / 0.2108 (a five-frame box: 0.2);
# from the pixels against the clean render: ratio 0.2386 / 0.2135 / 0.1975
MEASURED_FLICKER = {7: 0.2455, 11: 0.2201, 13: 0.2108}


@pytest.fixture(scope="module")
def clean_clip(oracle):
    """per seed: the clean 320 x 240 x 40 synth clip and the CPU oracle's measured transforms on it (made once, left unchanged)"""
    from video_stabilizer_amd import synth
    cache = {}

    def get(seed):
        if seed not in cache:
            clean, _ = synth.make_clip(320, 240, 40, seed=seed, channels=3)
            meas, succ, _, _ = EM.measure(oracle, clean, lag=10, crop_pixels=0)
            cache[seed] = (clean, meas, succ)
        return cache[seed]
    return get


@pytest.mark.parametrize("seed", (7, 11, 13))
def test_quality_pin_flicker(oracle, clean_clip, seed):
    """320 x 240 x 40 frames multiplied by seeded uniform gains g_k in 0.85 .. 1.15; ahead 4, step 4; the maps come from the CPU oracle's
    measured transforms on the CLEAN clip, so the figures do not depend on how the aligner copes with flicker.  Flicker = std of the successive
    differences of log(g_k G_k / 32768) (mean over the channels), frames 0 .. 35; also from the pixels: log(mean of the frame / mean of the clean
    render).  The bound is min(1.25 x this restatement's own figure, 0.5); a five-frame box gives 0.2."""
    O = oracle
    clean, meas, succ = clean_clip(seed)
    assert all(succ[1:])
    n = 36
    g = np.random.default_rng(seed + 1000).uniform(0.85, 1.15, len(clean))
    fl = np.clip(np.floor(clean.astype(np.float64) * g[:, None, None, None] + 0.5), 0, 255).astype(np.uint8)
    Gs = np.array([R.window_gains(O, fl, k, 4, meas, succ, 8, 4) for k in range(n)])
    assert (Gs[:, 3] == 4).all()
    before = np.std(np.diff(np.log(g[:n])))
    after = np.std(np.diff(np.log(g[:n, None] * Gs[:, :3] / 32768.0).mean(axis=1)))
    out = np.stack([R.apply_gain(fl[k], Gs[k], 255) for k in range(n)])

    def level(fr):
        return np.array([np.log(fr[i].astype(np.float64).mean() / clean[i].astype(np.float64).mean()) for i in range(n)])
    pb, pa = np.std(np.diff(level(fl[:n]))), np.std(np.diff(level(out)))
    print("seed %d: flicker before %.4f after %.4f ratio %.4f; from the pixels before %.4f after %.4f ratio %.4f" % (seed, before, after, after / before, pb, pa, pa / pb))
    bound = min(1.25 * MEASURED_FLICKER[seed], 0.5)
    assert after / before <= bound
    assert pa / pb <= bound


def pan_clip(n=40, w=320, h=240, pan=4):
    """a flicker-free clip panning at `pan` px per frame over a scene whose brightness rises along the pan (integer shifts: no resampling)"""
    from video_stabilizer_amd import synth
    W = w + pan * n + 8
    ramp = np.linspace(0.55, 1.0, W)[None, :]
    scene = np.stack([np.clip(np.floor(synth.base_texture(W, h, 21 + c) * 0.8 * ramp + 20.5), 0, 255) for c in range(3)], axis=-1).astype(np.uint8)
    return np.stack([scene[:, pan * k: pan * k + w] for k in range(n)])


def test_quality_pin_pan_and_direction(oracle):
    """A pan changes a frame's sum because the content changes: on a flicker-free pan of 4 px per frame along a brightness ramp the rule must invent
    less flicker (max |G - 32768| over frames 0 .. 35 and the channels) than whole-frame channel sums put through the same gain formula, and less
    than the rule with chain_j un-inverted (the direction pin).  Maps from the CPU oracle's measured transforms (it measures -3.85 px per frame,
    so the nearest samples are up to a pixel off the scene point: the rule's own figure is not 0).
    Measured with this restatement: the rule 227, whole-frame sums 876, wrong direction 1393 (of 32768: 0.7 %, 2.7 %, 4.3 %)."""
    O = oracle
    frames = pan_clip()
    meas, succ, _, _ = EM.measure(O, frames, lag=10, crop_pixels=0)
    assert all(succ[1:])

    def dev(**kw):
        Gs = [R.window_gains(O, frames, k, 4, meas, succ, 8, 4, **kw) for k in range(36)]
        assert all(G[3] == 4 for G in Gs)
        return max(abs(g - UNIT) for G in Gs for g in G[:3])
    rule, whole, flip = dev(), dev(whole=True), dev(mode="flip")
    print("max |G - 32768|: the rule %d, whole-frame sums %d, wrong direction %d" % (rule, whole, flip))
    assert rule < whole
    assert rule < flip


def test_parameter_boundary_symbols_and_default(vs):
    L = ctypes.CDLL(vs.LIB_PATH)
    for name in ("vs_deflicker_params_default", "vs_bgr_exposure_stats_batch", "vs_exposure_gains_batch", "vs_bgr_gain_batch",
                 "vs_stabilizer_set_deflicker", "vs_stabilizer_get_deflicker"):
        assert hasattr(L, name), name
        assert name in vs.SIGNATURES, name
    assert vs.ABI_VERSION == 5 and L.vs_abi_version() == 5
    assert vs.deflicker_params().step == 4
    # the boundary 0, 1, 64, 65 at the kernel-level entry points: the argument checks stand in front of any device work, so an accepted step gets
    # as far as the device (error -2 where there is none) and a refused one never does
    src = np.full((2, 4, 4, 3), 100, np.uint8)
    ts = [[vs.Transform.of(), vs.Transform.of()]]
    stats = np.zeros((1, 2, 8), np.uint64)
    for step, ok in ((0, False), (1, True), (64, True), (65, False), (-1, False)):
        p = vs.deflicker_params(step=step)
        for call in (lambda: vs.exposure_stats_batch(src, [[0, 1]], ts, params=p), lambda: vs.exposure_gains_batch(stats, 4, 4, params=p)):
            if ok:
                try:
                    call()
                except vs.VsError as e:
                    assert "error -2" in str(e), e
            else:
                with pytest.raises(vs.VsError, match="error -1"):
                    call()
    # a gain outside 16384 .. 65536 in host memory; statistics beyond the rule's bounds in host memory
    for bad in (16383, 65537, 0, 0xFFFFFFFF):
        with pytest.raises(vs.VsError, match="error -1"):
            vs.bgr_gain_batch(src, [[UNIT, bad, UNIT, 0], [UNIT, UNIT, UNIT, 0]])
    for k, v in ((0, 1 << 30), (1, 1 << 46), (6, 1 << 63)):
        s2 = stats.copy()
        s2[0, 1, k] = v
        with pytest.raises(vs.VsError, match="error -1"):
            vs.exposure_gains_batch(s2, 4, 4)
    # frames beyond 32767 a side, n_cand beyond 16, gray frames
    big = np.zeros((1, 1, 32768, 3), np.uint8)
    with pytest.raises(vs.VsError, match="error -3"):
        vs.exposure_stats_batch(big, [[0]], [[vs.Transform.of()]])
    with pytest.raises(vs.VsError, match="error -1"):
        vs.exposure_stats_batch(src, [[0] * 17], [[vs.Transform.of()] * 17])
    with pytest.raises(vs.VsError, match="error -1"):
        vs.exposure_stats_batch(src, [[0, 1]], ts, fmt=vs.FMT_GRAY8)
    with pytest.raises(vs.VsError, match="error -1"):
        vs.bgr_gain_batch(src, [[UNIT] * 4] * 2, fmt=vs.FMT_GRAY8)
