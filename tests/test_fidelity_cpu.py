"""-m "not gpu": THE FIDELITY RULE (vs_fidelity.hip, include/vs_amd.h) without a device -- the restatement (tests/_fidelity_ref.py) against values
computed by hand and against the direct float form (tests/_fidelity_direct.py), the rule's int32 bounds at the windows that reach them, the host
scores (vs_fidelity_scores) against Python's math, every argument check of vs_bgr_fidelity_batch, and the premise of the app test."""
import ctypes as C
import math

import numpy as np
import pytest

import _fidelity_direct as D
import _fidelity_ref as R


def _const(w, h, v, dtype=np.uint8):
    return np.full((h, w, 3), v, dtype)


def _checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    c = (((xx + yy) & 1) * 255).astype(np.uint8)
    return np.repeat(c[:, :, None], 3, axis=2)


# ---- the consequences, by hand ----------------------------------------------------------------------------------------------------
def test_a_identical_images():
    rng = np.random.default_rng(1)
    for (w, h), bits, dtype in (((21, 13), 8, np.uint8), ((8, 8), 10, np.uint16), ((5, 30), 16, np.uint16)):
        a = rng.integers(0, 1 << bits, (h, w, 3)).astype(dtype)
        nwx, nwy = R.n_windows(w, h)
        assert R.pair_stats(a, a, bits) == [0, 0, 0, 0, nwx * nwy, 65536 * nwx * nwy]
    assert R.n_windows(21, 13) == (4, 2) and R.n_windows(8, 8) == (1, 1) and R.n_windows(5, 30) == (0, 6) and R.n_windows(7, 7) == (0, 0)
    assert R.n_windows(11, 12) == (1, 2) and R.n_windows(32767, 32767) == (8190, 8190) and 8190 * 8190 < 1 << 26


def test_b_constant_100_against_130():
    """gray of (v, v, v) is v: the weights sum to 32768.  One window: s1 = 6400, s2 = 8320, ss = 64 (10000 + 16900) = 1 721 600, s12 = 832 000, so
    vars = 110 182 400 - 40 960 000 - 69 222 400 = 0 and cov = 53 248 000 - 53 248 000 = 0; A = 106 522 634, C = 110 209 034, B = D = c2:
    q = rint(65536 * 106522634 / 110209034) = rint(63343.9...) = 63344"""
    assert 3735 + 19235 + 9798 == 32768
    assert R.factors(6400, 8320, 1721600, 832000) == (0, 0, 106522634, 239708, 110209034, 239708)
    assert round(65536 * 106522634 / 110209034) == 63344 and abs(65536 * 106522634 / 110209034 - 63344) < 0.2
    w, h = 23, 14
    nw = 4 * 2
    assert R.pair_stats(_const(w, h, 100), _const(w, h, 130), 8) == [900 * w * h] * 4 + [nw, 63344 * nw]


@pytest.mark.parametrize("bits,dtype", [(8, np.uint8), (10, np.uint16), (12, np.uint16), (16, np.uint16)])
def test_c_all_zero_against_all_maximum(bits, dtype):
    """s1 = 0, s2 = 16320, ss = 64 * 65025 = 4 161 600: vars = 266 342 400 - 16320^2 = 0, cov = 0, A = c1, C = 266 342 400 + c1 = 266 369 034,
    B = D: q = rint(65536 * 26634 / 266369034) = rint(6.55...) = 7"""
    maxv = (1 << bits) - 1
    assert 16320 * 16320 == 266342400 == 64 * 4161600
    assert R.factors(0, 16320, 4161600, 0) == (0, 0, 26634, 239708, 266369034, 239708)
    assert 6.5 < 65536 * 26634 / 266369034 < 6.6
    w, h = 16, 9
    top = 65535 if bits > 8 else 255                                    # above the format's maximum where the container allows: the maximum
    for hi in (maxv, top):
        assert R.pair_stats(_const(w, h, 0, dtype), _const(w, h, hi, dtype), bits) == [maxv * maxv * w * h] * 3 + [65025 * w * h, 3, 7 * 3]


def test_d_checkerboard_against_its_inverse():
    """every window holds 32 samples of 255 on either side and no pixel where both are lit: s1 = s2 = 8160, ss = 4 161 600, s12 = 0;
    vars = 266 342 400 - 2 * 66 585 600 = 133 171 200, cov = -66 585 600; A = C = 133 197 834, B = -132 931 492, D = 133 410 908:
    q = rint(-65536 * 132931492 / 133410908) = rint(-65300.49...) = -65300"""
    assert R.factors(8160, 8160, 4161600, 0) == (133171200, -66585600, 133197834, -132931492, 133197834, 133410908)
    assert 65300.4 < 65536 * 132931492 / 133410908 < 65300.5
    w, h = 17, 12
    a = _checker(w, h)
    got = R.pair_stats(a, 255 - a, 8)
    assert got[:5] == [65025 * w * h] * 4 + [3 * 2]
    assert R.ssim_sum_signed(got[5]) == -65300 * 6 and got[5] > 1 << 63


def test_e_exchanging_the_images_changes_no_word():
    rng = np.random.default_rng(2)
    for bits, dtype in ((8, np.uint8), (12, np.uint16)):
        a = rng.integers(0, 1 << bits, (19, 26, 3)).astype(dtype)
        b = rng.integers(0, 1 << bits, (19, 26, 3)).astype(dtype)
        assert R.pair_stats(a, b, bits) == R.pair_stats(b, a, bits)


def test_pixels_outside_every_window_still_count_in_the_sse_words():
    a, b = _const(11, 9, 10), _const(11, 9, 10)
    b[8, 10] = (13, 14, 15)                                             # right of and below the only window
    got = R.pair_stats(a, b, 8)
    gy = int(R.gray(b, 8)[8, 10]) - 10
    assert got == [9, 16, 25, gy * gy, 1, 65536] and gy == 4


# ---- the int32 bounds ----------------------------------------------------------------------------------------------------------------
def test_int32_bounds_at_the_windows_that_reach_them():
    cases = {"all 255 on both sides": (16320, 16320, 8323200, 4161600), "0 against 255": (0, 16320, 4161600, 0),
             "checkerboard against its inverse": (8160, 8160, 4161600, 0), "checkerboard against itself": (8160, 8160, 4161600, 2080800)}
    worst = 0
    for name, sums in cases.items():
        f = R.factors(*sums)
        worst = max(worst, max(abs(v) for v in f))
        assert all(abs(v) <= R.LIMIT for v in f), name
        assert abs(f[2] * f[3]) < 1 << 59 and f[4] * f[5] < 1 << 59 and f[4] >= R.C1 and f[5] >= R.C2, name
        assert abs(int(R.window_q(*sums))) <= 65536
    assert R.LIMIT == 64 * 8323200 + R.C2 < 1 << 31 and worst == 532711434      # all-255: A = C = 2 * 16320^2 + c1
    # the largest D: vars at its maximum, both sides half 0 and half 255 -- vars = 64 * 4161600 - 2 * 8160^2 = 133 171 200 (far below the bound,
    # which takes 64 ss and drops the squares)
    assert R.factors(8160, 8160, 4161600, 2080800)[0] == 133171200
    rng = np.random.default_rng(3)
    ga, gb = rng.integers(0, 256, (40, 44)), rng.integers(0, 256, (40, 44))
    R.window_q(*R.window_sums(ga, gb))                                   # (asserts the bounds on 90 random windows)


# ---- the restatement against the direct form ---------------------------------------------------------------------------------------------
def test_restatement_agrees_with_the_direct_form():
    """within 2^-16: half a quantisation step (2^-17) plus what the rounding of c1 and c2 moves"""
    rng = np.random.default_rng(4)
    worst = 0.0
    for k in range(300):
        kind = k % 3
        ga = rng.integers(0, 256, (8, 8))
        gb = rng.integers(0, 256, (8, 8)) if kind == 0 else np.clip(ga + rng.integers(-12, 13, (8, 8)), 0, 255) if kind == 1 else \
            np.clip(ga // 2 + rng.integers(0, 30), 0, 255)
        q = int(R.window_q(*R.window_sums(ga, gb))[0, 0])
        worst = max(worst, abs(q / 65536.0 - D.ssim_window(ga, gb)))
    print("worst gap over 300 windows: %.3g" % worst)
    assert worst <= 2.0 ** -16


# ---- the host scores -----------------------------------------------------------------------------------------------------------------
FMT_BITS = {1: 8, 2: 10, 3: 12, 4: 16}


def test_scores_against_python_math(vs):
    rng = np.random.default_rng(5)
    for fmt, bits in FMT_BITS.items():
        w, h = 1920, 1080
        st = np.zeros((40, 6), np.uint64)
        st[:, :4] = rng.integers(1, 1 << 40, (40, 4))
        st[:, 4] = rng.integers(1, 1 << 20, 40)
        st[:, 5] = (rng.integers(-65536, 65537, 40) * st[:, 4].astype(np.int64)).astype(np.int64).view(np.uint64)
        got = vs.fidelity_scores(st, w, h, fmt)
        for i in range(40):
            want = R.scores(st[i], w, h, bits)
            assert got[i].tolist() == pytest.approx(want, rel=1e-12), (fmt, i)
    # the consequences through the scores: 100 against 130 is 10 log10(255^2 / 900) dB; SSIM 63344 / 65536
    s = vs.fidelity_scores(np.array([R.pair_stats(_const(16, 16, 100), _const(16, 16, 130), 8)], np.uint64), 16, 16, 1)[0]
    assert s[:5].tolist() == pytest.approx([10.0 * math.log10(65025.0 / 900.0)] * 5, rel=1e-12) and s[5] == 63344.0 / 65536.0
    s = vs.fidelity_scores(np.array([R.pair_stats(_checker(16, 16), 255 - _checker(16, 16), 8)], np.uint64), 16, 16, 1)[0]
    assert s[:5].tolist() == [0.0] * 5 and s[5] == -65300.0 / 65536.0


def test_zero_sse_is_huge_val_and_no_window_is_nan(vs):
    got = vs.fidelity_scores(np.array([[0, 0, 0, 0, 9, 9 * 65536], [0, 5, 0, 7, 0, 0]], np.uint64), 7, 40, 1)
    assert np.isposinf(got[0, :5]).all() and got[0, 5] == 1.0
    assert np.isposinf(got[1, [0, 2]]).all() and np.isfinite(got[1, [1, 3, 4]]).all() and np.isnan(got[1, 5])
    assert vs.fidelity_scores(np.zeros((0, 6), np.uint64), 8, 8).shape == (0, 6)


def test_scores_argument_checks(vs):
    st = np.ones((1, 6), np.uint64)
    out = (vs.FidelityScore * 1)()
    f = vs.lib().vs_fidelity_scores
    assert f(vs._p(st), 1, 8, 8, 1, out) == 0
    for args in ((vs._p(st), -1, 8, 8, 1, out), (vs._p(st), 1, 0, 8, 1, out), (vs._p(st), 1, 8, 32768, 1, out), (vs._p(st), 1, 8, 8, 0, out),
                 (vs._p(st), 1, 8, 8, 99, out), (None, 1, 8, 8, 1, out), (vs._p(st), 1, 8, 8, 1, None)):
        assert f(*args) == -1, args[1:5]
        assert "vs_fidelity_scores" in vs.lib().vs_last_error().decode()


# ---- vs_bgr_fidelity_batch's argument checks: all of them before any device work ------------------------------------------------------
def test_every_argument_check_without_a_device(vs):
    w, h, n = 16, 12, 3
    a = np.zeros((n, h, w, 3), np.uint8)
    st = np.zeros((4, 6), np.uint64)
    pairs = np.array([[0, 1], [2, 2]], np.int32)
    f = vs.lib().vs_bgr_fidelity_batch
    ip = C.POINTER(C.c_int32)

    def call(**kw):
        d = dict(a=vs._p(a), a_fs=h * w * 3, n_a=n, a_stride=w * 3, b=vs._p(a), b_fs=h * w * 3, n_b=n, b_stride=w * 3, w=w, h=h, fmt=1, n_pairs=2,
                 pairs=pairs.ctypes.data_as(ip), stats=vs._p(st), mem=vs.MEM_HOST)
        d.update(kw)
        return f(d["a"], d["a_fs"], d["n_a"], d["a_stride"], d["b"], d["b_fs"], d["n_b"], d["b_stride"], d["w"], d["h"], d["fmt"], d["n_pairs"], d["pairs"],
                 d["stats"], d["mem"], None)

    keep = []

    def idx(*v):
        keep.append(np.array(v, np.int32))
        return keep[-1].ctypes.data_as(ip)
    bad = [dict(w=0), dict(h=0), dict(w=32768, a_stride=3 * 32768, b_stride=3 * 32768), dict(h=32768), dict(fmt=0), dict(fmt=77), dict(a=None), dict(b=None),
           dict(n_a=0), dict(n_b=0), dict(n_pairs=-1), dict(a_stride=3 * w - 1), dict(b_stride=3 * w - 1), dict(a_fs=(h - 1) * w * 3 + 3 * w - 1),
           dict(b_fs=0), dict(pairs=None), dict(stats=None), dict(pairs=idx(0, 1, 3, 0)), dict(pairs=idx(0, 1, 0, 3)), dict(pairs=idx(-1, 0, 0, 0)),
           dict(pairs=idx(0, 0, 0, -1)), dict(n_b=1, pairs=idx(0, 0, 0, 1))]
    for kw in bad:
        for mem in (vs.MEM_HOST, vs.MEM_DEVICE):
            assert call(mem=mem, **kw) == -1, kw
            assert "bad argument" in vs.lib().vs_last_error().decode(), kw
    # no pairs: VS_OK, whatever the pair and statistics pointers are, and nothing is written
    st[:] = 7
    assert call(n_pairs=0, pairs=None, stats=None) == 0 and call(n_pairs=0) == 0 and (st == 7).all()
    # one frame a side: the frame stride is not looked at
    if vs.device_count() < 1:
        assert call(n_a=1, n_b=1, a_fs=0, b_fs=0, pairs=idx(0, 0, 0, 0)) == -2       # past every check: only the device is missing
        assert "no usable HIP device" in vs.lib().vs_last_error().decode()


def test_both_symbols_are_present(vs):
    L = C.CDLL(vs.LIB_PATH)
    assert hasattr(L, "vs_bgr_fidelity_batch") and hasattr(L, "vs_fidelity_scores")
    assert "vs_bgr_fidelity_batch" in vs.SIGNATURES and "vs_fidelity_scores" in vs.SIGNATURES
    assert C.sizeof(vs.FidelityScore) == 48
    assert callable(vs.fidelity_stats_batch) and callable(vs.fidelity_stats_batch_device) and callable(vs.fidelity_scores)


def test_the_program_is_built_and_never_falls_back(vs, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "apps"), "-s", "-j4"])
    prog = os.path.join(root, "apps", "bin", "vs_eval_fidelity")
    r = subprocess.run([prog], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Usage:" in r.stderr and "--inset C" in r.stderr and "--ref clip" in r.stderr
    if vs.device_count() < 1:
        np.zeros((3, 16, 16, 3), np.uint8).tofile(tmp_path / "clip_16x16.bgr")
        r = subprocess.run([prog, str(tmp_path / "clip_16x16.bgr")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "No HIP device" in r.stderr and r.stdout == ""


# ---- the premise of the app test ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 4])
def test_a_steady_clip_scores_above_its_shaken_twin(seed):
    """the same scene under the same pan, with and without jitter: ITF (dB) and mean SSIM of the frames minus 16 pixels a side"""
    from video_stabilizer_amd import synth
    shaken, _ = synth.make_clip(160, 128, 12, seed, channels=3, pan=0.5, jitter_t=4.0)
    steady, _ = synth.make_clip(160, 128, 12, seed, channels=3, pan=0.5, jitter_t=0.0, jitter_b=0.0, jitter_a=0.0)
    p_sh, y_sh, s_sh = R.itf(shaken, 8, 16)
    p_st, y_st, s_st = R.itf(steady, 8, 16)
    print("seed %d: shaken ITF %.2f dB (gray %.2f), SSIM %.4f; steady ITF %.2f dB (gray %.2f), SSIM %.4f" % (seed, p_sh, y_sh, s_sh, p_st, y_st, s_st))
    assert p_st > p_sh and y_st > y_sh and s_st > s_sh
