"""THE RESIZE RULE without a device (include/vs_amd.h: vs_resize_taps, vs_bgr_resize_batch; csrc/vs_resize.hpp): the rule's consequences (a) to
(g) on the restatement (tests/_resize_ref.py), the library's host tables against the restatement over the sweep, the restatement against the
ideal it approximates (tests/_resize_direct.py) under a bound derived from the rule, every argument error, symbols and defaults."""
import ctypes as C
from fractions import Fraction as Fr

import numpy as np
import pytest

import _resize_direct as D
import _resize_ref as R

FILTERS = [R.LINEAR, R.AREA]


def destinations(s):
    """a dozen destination extents for a source extent: both sides of 1:1, 2:1 and the 8:1 limit, up and down, the ends of the range"""
    c = {1, 2, 3, s - 1, s, s + 1, 2 * s, (s + 1) // 2, s // 2, (s + 7) // 8, (s + 7) // 8 - 1, (3 * s) // 2, (2 * s) // 3, 4 * s, 32767 if s > 4000 else 7 * s + 3}
    return sorted(d for d in c if 1 <= d <= 32767)[:14]


def rnd(shape, maxv, seed, dtype):
    return np.random.default_rng(seed).integers(0, maxv + 1, shape).astype(dtype)


# ---- the consequences, on the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype,maxv", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_a_the_same_size_is_the_identity(filt, dtype, maxv):
    src = rnd((2, 9, 13, 3), maxv, 1, dtype)
    assert np.array_equal(R.resize(src, 13, 9, filt, maxv), src)
    for s in (1, 2, 7, 199, 3840):
        i0, n, wt = R.table(s, s, filt)
        assert np.array_equal(i0, np.arange(s)) and (n == 1).all() and (wt[:, 0] == 4096).all()


@pytest.mark.parametrize("filt", FILTERS)
def test_b_a_constant_frame_stays_constant(filt):
    for value, dtype, maxv in ((0, np.uint8, 255), (255, np.uint8, 255), (77, np.uint8, 255), (1023, np.uint16, 1023), (65535, np.uint16, 65535)):
        src = np.full((1, 16, 24, 3), value, dtype)
        for dw, dh in ((24, 16), (12, 8), (7, 5), (3, 2), (24, 9)) + (((31, 40), (96, 64)) if filt == R.LINEAR else ()):
            assert (R.resize(src, dw, dh, filt, maxv) == value).all(), (value, dw, dh)


@pytest.mark.parametrize("filt", FILTERS)
def test_c_every_output_lies_within_its_taps(filt):
    maxv = 1023
    src = rnd((1, 11, 17, 3), 65535, 2, np.uint16)             # samples above the maximum: they count as the maximum
    clipped = np.minimum(src, maxv)
    for dw, dh in ((5, 4), (17, 6), (9, 11), (3, 2)) + (((23, 30),) if filt == R.LINEAR else ()):
        out = R.resize(src, dw, dh, filt, maxv)
        assert out.max() <= maxv
        xi, xn, _ = R.table(17, dw, filt)
        yi, yn, _ = R.table(11, dh, filt)
        for e in range(dh):
            for d in range(dw):
                win = clipped[0, yi[e]:yi[e] + yn[e], xi[d]:xi[d] + xn[d]].reshape(-1, 3)
                assert (out[0, e, d] >= win.min(0)).all() and (out[0, e, d] <= win.max(0)).all(), (dw, dh, e, d)


def test_d_area_at_an_integer_factor_has_equal_weights():
    for k in (2, 4, 8):
        for dn in (1, 5, 480):
            i0, n, wt = R.table(k * dn, dn, R.AREA)
            assert np.array_equal(i0, k * np.arange(dn)) and (n == k).all() and (wt[:, :k] == 4096 // k).all() and (wt[:, k:] == 0).all()
    src = rnd((1, 10, 14, 3), 255, 3, np.uint8).astype(np.int64)
    want = (src[:, 0::2, 0::2] + src[:, 0::2, 1::2] + src[:, 1::2, 0::2] + src[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize(src.astype(np.uint8), 7, 5, R.AREA, 255), want)


def test_e_linear_at_two_to_one_equals_area():
    for dn in (1, 3, 960, 1920):
        for a, b in zip(R.table(2 * dn, dn, R.LINEAR), R.table(2 * dn, dn, R.AREA)):
            assert np.array_equal(a, b)
    src = rnd((1, 12, 18, 3), 4095, 4, np.uint16)
    assert np.array_equal(R.resize(src, 9, 6, R.LINEAR, 4095), R.resize(src, 9, 6, R.AREA, 4095))


def test_f_linear_four_to_eight():
    i0, n, wt = R.table(4, 8, R.LINEAR)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3]
    assert [wt[d, :n[d]].tolist() for d in range(8)] == [[4096], [3072, 1024], [1024, 3072], [3072, 1024], [1024, 3072], [3072, 1024], [1024, 3072], [4096]]


def test_g_area_seven_to_three():
    i0, n, wt = R.table(7, 3, R.AREA)
    assert i0.tolist() == [0, 2, 4]
    assert [wt[d, :n[d]].tolist() for d in range(3)] == [[1755, 1756, 585], [1170, 1756, 1170], [585, 1756, 1755]]


def test_four_k_to_1080_has_no_zero_weight():
    for s, dn in ((3840, 1080), (3840, 1920), (2160, 1080)):
        i0, n, wt = R.table(s, dn, R.AREA)
        assert all((wt[d, :n[d]] > 0).all() for d in range(dn))


# ---- the library's host tables against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
def test_the_library_s_tables_are_the_restatement_s_over_the_sweep(vs, filt):
    pairs = 0
    for s in R.SWEEP_SIZES:
        for dn in destinations(s):
            if not R.axis_valid(s, dn, filt):
                with pytest.raises(vs.VsError, match="error -3"):
                    vs.resize_taps(s, dn, filt)
                continue
            i0, n, wt = vs.resize_taps(s, dn, filt)
            ri0, rn, rwt = R.table(s, dn, filt)
            assert np.array_equal(i0, ri0) and np.array_equal(n, rn) and np.array_equal(wt, rwt), (s, dn)
            # what the rule promises of every table
            assert (wt.astype(np.int64).sum(1) == 4096).all() and (n >= 1).all() and (n <= 9).all() and (i0 >= 0).all() and (i0 + n <= s).all(), (s, dn)
            pairs += 1
    assert pairs > 1000


# ---- the restatement against the ideal -------------------------------------------------------------------------------------------------
CASES = [(7, 5, 3, 2), (8, 8, 4, 4), (16, 3, 2, 3), (9, 6, 9, 2), (5, 16, 4, 2), (6, 4, 5, 3)]
UP = [(4, 3, 8, 7), (5, 4, 6, 17), (3, 7, 11, 2), (1, 1, 5, 3), (6, 9, 4, 13)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("dtype,maxv", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_the_restatement_is_within_the_rule_s_own_error_of_the_ideal(filt, dtype, maxv):
    """The bound comes from the rule, not from a measurement.  A table weight differs from the ideal weight by less than 1 / 4096: LINEAR's f is
    the ideal fraction floored to 1 / 4096 (and 4096 - f its complement); AREA's C_k are the ideal running sums rounded to the nearest
    1 / 4096, at most a half off each, and the ties all round the same way, so a difference of two is less than 1 off.  With the ideal weights
    ax, ay (each axis sums to 1, as the table's do) and the table's wx, wy:  sum |wx wy - ax ay| <= sum_k |wx_k - ax_k| + sum_j |wy_j - ay_j|
    < (nx + ny) / 4096, nx and ny the taps of either side (LINEAR: 2, AREA: the table's count).  Every sample is at most max_value, and the
    final shift rounds to nearest: a half more."""
    for sw, sh, dw, dh in CASES + (UP if filt == R.LINEAR else []):
        if not (R.axis_valid(sw, dw, filt) and R.axis_valid(sh, dh, filt)):
            continue
        src = rnd((1, sh, sw, 3), maxv, sw * 31 + dh, dtype)
        src[0, 0, 0] = maxv
        src[0, -1, -1] = 0
        got = R.resize(src, dw, dh, filt, maxv)[0]
        ideal = D.resize(src[0].tolist(), dw, dh, filt, maxv)
        nx = 2 if filt == R.LINEAR else int(R.table(sw, dw, filt)[1].max())
        ny = 2 if filt == R.LINEAR else int(R.table(sh, dh, filt)[1].max())
        bound = Fr(1, 2) + Fr(maxv * (nx + ny), 4096)
        worst = max(abs(int(got[e, d, c]) - ideal[e][d][c]) for e in range(dh) for d in range(dw) for c in range(3))
        print("%dx%d -> %dx%d filter %d max %d: worst %.4f, bound %.4f" % (sw, sh, dw, dh, filt, maxv, float(worst), float(bound)))
        assert worst <= bound, (sw, sh, dw, dh, float(worst), float(bound))


def test_the_ideal_s_weights_sum_to_one():
    for filt in FILTERS:
        for s, dn in ((7, 3), (8, 1), (16, 2), (5, 5)) + (((3, 11), (1, 4)) if filt == R.LINEAR else ()):
            for d in range(dn):
                assert sum(D.axis_weights(s, dn, filt, d).values()) == 1


# ---- argument errors: every one comes back before a device is asked for ----------------------------------------------------------------
def _call(vs, src, n, sw, sh, ss, fmt, filt, dst, dw, dh, ds, mem=0, sfs=None, dfs=None):
    return vs.lib().vs_bgr_resize_batch(vs._p(src) if src is not None else None, sh * ss if sfs is None else sfs, n, sw, sh, ss, fmt, filt,
                                        vs._p(dst) if dst is not None else None, dh * ds if dfs is None else dfs, dw, dh, ds, mem, None)


def _err(vs):
    return vs.lib().vs_last_error().decode()


def test_the_batch_call_s_argument_errors(vs):
    src, dst = np.zeros((2, 6, 8 * 3), np.uint8), np.zeros((2, 4, 5 * 3), np.uint8)
    ok = dict(src=src, n=2, sw=8, sh=6, ss=24, fmt=vs.FMT_BGR8, filt=vs.RESIZE_LINEAR, dst=dst, dw=5, dh=4, ds=15)
    bad = [dict(src=None), dict(dst=None), dict(dst=src), dict(n=-1), dict(sw=0), dict(sh=0), dict(dw=0), dict(dh=0), dict(sw=-3), dict(dw=70000),
           dict(ss=23), dict(ds=14), dict(fmt=vs.FMT_GRAY8), dict(fmt=99), dict(filt=2), dict(filt=-1), dict(mem=2), dict(sfs=6 * 24 - 1), dict(dfs=4 * 15 - 1)]
    for b in bad:
        assert _call(vs, **dict(ok, **b)) == -1, b
        assert "vs_bgr_resize_batch" in _err(vs) or "bad argument" in _err(vs), _err(vs)
    # beyond 32767 a side, and AREA outside its range with the axis named: unsupported, before any work
    assert _call(vs, **dict(ok, sw=32768, ss=3 * 32768)) == -3 and "32767" in _err(vs)
    assert _call(vs, **dict(ok, dh=32768)) == -3
    assert _call(vs, **dict(ok, filt=vs.RESIZE_AREA, dw=9, ds=27)) == -3 and "x axis" in _err(vs)                  # up on x
    assert _call(vs, **dict(ok, filt=vs.RESIZE_AREA, sw=41, ss=123, dw=5)) == -3 and "x axis" in _err(vs)          # one past 8:1
    assert _call(vs, **dict(ok, filt=vs.RESIZE_AREA, dh=7)) == -3 and "y axis" in _err(vs)
    # no frames: VS_OK, nothing launched, no device asked for; the pointers are not looked at
    assert _call(vs, **dict(ok, n=0)) == 0
    assert _call(vs, **dict(ok, n=0, src=None, dst=None)) == 0
    assert _call(vs, **dict(ok, n=0, filt=vs.RESIZE_AREA, dw=9, ds=27)) == -3


def test_the_table_call_s_argument_errors(vs):
    i0, n, wt = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros((8, 10), np.uint16)
    f = vs.lib().vs_resize_taps
    assert f(4, 8, vs.RESIZE_LINEAR, vs._p(i0), vs._p(n), vs._p(wt)) == 0
    for args in ((0, 8, 0), (4, 0, 0), (32768, 8, 0), (4, 32768, 0), (4, 8, 2), (4, 8, -1)):
        assert f(*args, vs._p(i0), vs._p(n), vs._p(wt)) == -1, args
    assert f(4, 8, 0, None, vs._p(n), vs._p(wt)) == -1 and f(4, 8, 0, vs._p(i0), None, vs._p(wt)) == -1 and f(4, 8, 0, vs._p(i0), vs._p(n), None) == -1
    assert f(4, 8, vs.RESIZE_AREA, vs._p(i0), vs._p(n), vs._p(wt)) == -3                                                # AREA does not enlarge
    assert f(65, 8, vs.RESIZE_AREA, vs._p(i0), vs._p(n), vs._p(wt)) == -3 and f(64, 8, vs.RESIZE_AREA, vs._p(i0), vs._p(n), vs._p(wt)) == 0


def test_the_table_call_writes_unused_weights_as_zero(vs):
    wt = np.full((3, 10), 0xabcd, np.uint16)
    i0, n = np.zeros(3, np.int32), np.zeros(3, np.int32)
    assert vs.lib().vs_resize_taps(7, 3, vs.RESIZE_AREA, vs._p(i0), vs._p(n), vs._p(wt)) == 0
    assert n.tolist() == [3, 3, 3] and (wt[:, 3:] == 0).all() and wt[0, :3].tolist() == [1755, 1756, 585]


def test_symbols_and_defaults(vs):
    L = C.CDLL(vs.LIB_PATH)
    for name in ("vs_resize_taps", "vs_bgr_resize_batch"):
        assert hasattr(L, name) and name in vs.SIGNATURES
    assert (vs.RESIZE_LINEAR, vs.RESIZE_AREA) == (0, 1) == (R.LINEAR, R.AREA) == (D.LINEAR, D.AREA)
    assert vs.lib().vs_abi_version() == 5
