"""Phase-correlation initialisation, CPU side: the oracle's restatement of cv::phaseCorrelate (oracle/vs_phase.cpp)
against independent arithmetic (numpy's double-precision FFT) and hand-derivable answers.  Parity unpinned with respect
to OpenCV itself (not in the image); what is pinned is the published structure and its observable properties."""
import numpy as np
import pytest


# cv::getOptimalDFTSize: smallest 2^a 3^b 5^c >= n
OPTIMAL_DFT_SIZE = {1: 1, 2: 2, 7: 8, 11: 12, 13: 15, 17: 18, 61: 64, 80: 80, 97: 100, 120: 120, 135: 135, 270: 270, 271: 288,
                    480: 480, 481: 486, 540: 540, 960: 960, 1081: 1125, 4097: 4320}


def test_optimal_dft_size(oracle):
    for n, w in OPTIMAL_DFT_SIZE.items():
        assert oracle.optimal_dft_size(n) == w, n
    assert oracle.optimal_dft_size(0) == -1


def test_optimal_dft_size_of_the_product_library(vs):
    # host-side function of the product library, same rule (a test of its own: tests/test_oracle_sanitizers.py runs this file's oracle
    # tests in a sanitizer process that must not load the product library and its HIP runtime)
    for n, w in OPTIMAL_DFT_SIZE.items():
        assert vs.optimal_dft_size(n) == w, n
    assert vs.optimal_dft_size(0) == -1


def test_radix_plan_rule(oracle):
    # fives, then threes, then fours, then at most one two (the order fixes the rounding, so it is part of the contract)
    assert oracle.fft_plan(480) == [5, 3, 4, 4, 2]
    assert oracle.fft_plan(270) == [5, 3, 3, 3, 2]
    assert oracle.fft_plan(960) == [5, 3, 4, 4, 4]
    assert oracle.fft_plan(540) == [5, 3, 3, 3, 4]
    assert oracle.fft_plan(1) == []
    assert oracle.fft_plan(64) == [4, 4, 4]
    assert oracle.fft_plan(7) is None and oracle.fft_plan(22) is None


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 20, 25, 27, 30, 45, 64, 75, 80, 120, 135, 160, 270, 480, 540, 960, 1920, 4096])
def test_fft_matches_numpy(oracle, n):
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    ref = np.fft.fft(x.astype(np.complex128))
    y = oracle.fft_c2c(x)
    assert np.abs(y - ref).max() <= 3e-6 * max(1.0, np.abs(ref).max())
    back = oracle.fft_c2c(y, inverse=True) / n            # the inverse is unscaled, like cv::idft without DFT_SCALE
    assert np.abs(back - x).max() <= 1e-5
    # an impulse transforms to all ones exactly; a constant to n at bin 0 and exact zeros elsewhere for power-of-two n
    e = np.zeros(n, np.complex64)
    e[0] = 1
    assert np.array_equal(oracle.fft_c2c(e), np.ones(n, np.complex64))


def _texture(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(270, 480), (120, 160), (64, 80), (135, 240)])
def test_circular_shift_is_recovered(oracle, shape):
    # b(x) = a(x - d)  ->  phaseCorrelate(a, b) = +d with response 1 (the whole energy sits in one sample)
    # (for an odd extent the centre is extent / 2.0 while the zero-shift peak lands on sample extent // 2: the published
    # formula then reports +0.5 -- kept, since the reference would see the same from OpenCV)
    a = _texture(*shape, seed=3)
    ox, oy = 0.5 * (shape[1] % 2), 0.5 * (shape[0] % 2)
    for dx, dy in [(0, 0), (3, -2), (-7, 5), (20, 11), (-1, 0)]:
        b = np.roll(a, (dy, dx), (0, 1))
        sx, sy, r = oracle.phase_correlate(a, b)
        assert abs(sx - dx - ox) < 1e-5 and abs(sy - dy - oy) < 1e-5, (dx, dy, sx, sy)
        assert abs(r - 1.0) < 1e-5


def test_surface_matches_double_precision(oracle):
    a = _texture(270, 480, seed=5).astype(np.float32)
    b = np.roll(a, (4, -3), (0, 1))
    Fa, Fb = np.fft.fft2(a.astype(np.float64)), np.fft.fft2(b.astype(np.float64))
    P = Fa * np.conj(Fb)
    ref = np.real(np.fft.ifft2(P / np.abs(P))) * a.size           # unscaled inverse
    s = oracle.phase_surface(a, b)
    assert s.shape == (270, 480)
    assert np.abs(s - ref).max() < 1e-7 * a.size
    assert np.unravel_index(s.argmax(), s.shape) == (270 - 4, 3)   # unshifted: the peak sits at -d modulo the extent


def test_padding_and_float_input(oracle):
    # 61 x 97 is padded to 64 x 100 with zeros: the shift of the content is still found (response drops below 1)
    big = _texture(200, 200, seed=9)
    a = big[50:111, 40:137]
    b = big[48:109, 43:140]            # content moved by (-3, +2)
    sx, sy, r = oracle.phase_correlate(a, b)
    assert abs(sx + 3) < 0.2 and abs(sy - 2) < 0.2 and 0.3 < r < 1.0
    s = oracle.phase_surface(a.astype(np.float32), b.astype(np.float32))
    assert s.shape == (64, 100)
    assert oracle.phase_correlate(a.astype(np.float32), b.astype(np.float32)) == (sx, sy, r)


def test_subpixel_centroid(oracle):
    # two equal neighbouring samples -> centroid half way; response = their sum / (M N)
    s = np.zeros((64, 80), np.float32)
    s[0, 0] = 100.0       # shifted position (32, 40): the centre -> shift 0
    s[0, 1] = 100.0       # shifted (32, 41)
    dx, dy, r = oracle.phase_peak(s)
    assert abs(dx + 0.5) < 1e-9 and abs(dy) < 1e-9 and abs(r - 200.0 / (64 * 80)) < 1e-12
    # ties: the first maximum in row-major order of the *shifted* image wins -> unshifted (M/2, N/2) comes first
    t = np.zeros((64, 80), np.float32)
    t[32, 40] = 5.0       # shifted (0, 0)
    t[0, 0] = 5.0         # shifted (32, 40)
    dx, dy, r = oracle.phase_peak(t)
    assert abs(dx - 40.0) < 1e-9 and abs(dy - 32.0) < 1e-9   # window clipped at the corner: only the (0,0) sample has weight
    # window clipping at the border keeps the centroid inside the image
    u = np.zeros((64, 80), np.float32)
    u[31, 39] = 1.0       # shifted (63, 79): bottom-right corner
    dx, dy, r = oracle.phase_peak(u)
    assert abs(dx - (40.0 - 79.0)) < 1e-9 and abs(dy - (32.0 - 63.0)) < 1e-9   # sum + DBL_EPSILON in the divisor


def test_aligner_uses_the_reference_scale(oracle):
    """alignment.cpp:380-386: TX = shift.x * (1 << PhaseLevel) / float(1 << PyramidLevels), negated on keyframes"""
    from video_stabilizer_amd import synth
    path = [(0, 0, 0, 0), (0.0, 0.0, 8.0, -4.0), (0.0, 0.0, 0.0, 0.0)]
    frames, _ = synth.make_clip(640, 480, 3, seed=4, path=path)
    a = oracle.Aligner(phase_correlate=1)
    ok0, _ = a.align_next(frames[0])
    ok1, t1 = a.align_next(frames[1])
    d = a.debug()
    assert not ok0 and ok1
    # level 2 is 160x120: an 8 px / -4 px motion is 2 / -1 px there (without a window the frame border, which does not
    # move, pulls the centroid towards zero)
    assert abs(abs(d.phase_dx) - 2.0) < 0.5 and abs(abs(d.phase_dy) - 1.0) < 0.25 and d.phase_response > 0.5, (d.phase_dx, d.phase_dy, d.phase_response)
    # The start value as the reference writes it: shift * 4 / 2^levels -- in units of a level below the coarsest one, i.e.
    # half the motion -- and negated when the current frame is the keyframe.  With OpenCV's documented sign (content moved
    # by +d from the first to the second image -> +d) that negation points the start value *away* from the solution the
    # loop then finds; the reference's README says of this mode "seems to make things worse (maybe a bug?)".  Kept as is:
    # the drop-in reproduces the reference, and the loop recovers (one extra iteration here).
    b = oracle.Aligner()
    b.align_next(frames[0])
    _, t1b = b.align_next(frames[1])
    lv = d.levels
    start_tx = -(d.phase_dx * np.float32(4.0 / (1 << lv)))     # frame 1 is the keyframe (alignment.cpp:383-386)
    assert start_tx * d.level_transform[lv - 1].TX < 0
    assert sum(d.iterations[:lv]) >= sum(b.debug().iterations[:lv])
    assert max(abs(x - y) for x, y in zip(t1.tup(), t1b.tup())) < 0.5
    # a threshold above any response disables the start value: bit-identical to phase_correlate off
    c = oracle.Aligner(phase_correlate=1, phase_correlate_threshold=2.0)
    c.align_next(frames[0])
    _, t1c = c.align_next(frames[1])
    assert t1c.tup() == t1b.tup()
