"""The rolling-shutter rule's restatement (tests/_rolling_ref.py) on the CPU: its blends against the oracle's VS_WARP_BILINEAR_CV warp, the
rule's consequences (a) - (e), a direct float64 form of the model, and the direction test against rendered rolling-shutter frames."""
import numpy as np
import pytest

import _fill_ref as FR
import _rolling_ref as R

MOTIONS = [(0.0, 0.0, 7.0, -3.0), (0.02, -0.03, 2.5, 1.25), (-0.01, 0.015, -4.0, 6.5)]


def _noise(rng, w, h, dtype, maxv):
    return rng.integers(0, maxv + 1, (h, w, 3)).astype(dtype)


@pytest.mark.parametrize("dtype,maxv", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_the_blend_restatement_is_the_oracle_s_warp_on_covered_pixels(oracle, dtype, maxv):
    O = oracle
    rng = np.random.default_rng(maxv)
    w, h = 61, 37
    frame = _noise(rng, w, h, dtype, maxv)
    seen = 0
    for tup in MOTIONS + [(0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.5, -1.5)]:
        t = O.Transform.of(*tup)
        X0, Y0, ad, bd = FR._table_terms(O, t, w, h, FR.cv_round_sat)
        X, Y = FR.wrap32(FR.wrap32(X0 + 16) + ad) >> 5, FR.wrap32(FR.wrap32(Y0 + 16) + bd) >> 5
        cov = FR.covered(O, t, w, h)
        want = O.bgr_image_warp(frame, t, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=maxv)
        got = R.blend(frame, X, Y, maxv)
        assert cov.mean() > 0.5
        assert np.array_equal(got[cov], want[cov]), tup
        seen += int(((X & 31 != 0) | (Y & 31 != 0))[cov].sum())
    assert seen > 1000                                               # the comparison was about interpolated samples


@pytest.mark.parametrize("dtype,maxv", [(np.uint8, 255), (np.uint16, 1023), (np.uint16, 65535)])
def test_the_rule_s_consequences(oracle, dtype, maxv):
    O = oracle
    rng = np.random.default_rng(7 + maxv)
    for w, h in ((33, 21), (64, 16), (5, 1), (1, 7)):
        frame = _noise(rng, w, h, dtype, maxv)
        for tup in MOTIONS:
            M = O.cv_inverse_matrix(O.Transform.of(*tup), w, h)
            # (a) no motion, (b) rho == 0, (c) a motion of {0, 0, 0, 0}
            assert np.array_equal(R.rolling_frame(frame, None, 0.7, maxv), frame)
            assert np.array_equal(R.rolling_frame(frame, M, 0.0, maxv), frame)
            assert np.array_equal(R.rolling_frame(frame, M, -0.0, maxv), frame)
            ident = O.cv_inverse_matrix(O.Transform.of(0, 0, 0, 0), w, h)
            assert np.array_equal(np.asarray(ident, np.float64).reshape(6), [1, 0, 0, 0, 1, 0])
            for rho in (-1.0, 0.5, 1.0):
                assert np.array_equal(R.rolling_frame(frame, ident, rho, maxv), frame)
                out = R.rolling_frame(frame, M, rho, maxv)
                # (d) odd h: the middle row, whatever the motion
                if h % 2 == 1:
                    assert np.array_equal(out[(h - 1) // 2], frame[(h - 1) // 2]), (w, h, tup, rho)
                # (e) per channel between the frame's extremes
                for c in range(3):
                    assert frame[..., c].min() <= out[..., c].min() and out[..., c].max() <= frame[..., c].max()
                if w > 8 and h > 8:
                    assert (out != frame).mean() > 0.3               # the pass did something
    # (e) on a frame whose extremes are not the format's
    frame = (_noise(rng, 40, 30, dtype, maxv) // 3 + maxv // 4).astype(dtype)
    out = R.rolling_frame(frame, O.cv_inverse_matrix(O.Transform.of(*MOTIONS[1]), 40, 30), 1.0, maxv)
    assert frame.min() <= out.min() and out.max() <= frame.max() and (out != frame).any()


def test_row_times_and_the_direct_float64_model(oracle):
    O = oracle
    for h in (1, 2, 7, 64, 1080):
        tau = R.row_times(h, 1.0)
        assert np.allclose(tau, (np.arange(h) - (h - 1) / 2.0) / h, rtol=0, atol=1e-15)
        assert h % 2 == 0 or tau[(h - 1) // 2] == 0.0
        assert np.array_equal(R.row_times(h, -0.5), -0.5 * tau)
    # the rule's position against the model in plain float64: two cvRounds (half a unit of 1/1024 each), the + 16 and the shift by five bits
    # leave the position within (0.5 + 1 / 32) / 32 px of the real one; 1e-6 for the doubles' own rounding
    w, h = 193, 107
    for tup in MOTIONS:
        M = O.cv_inverse_matrix(O.Transform.of(*tup), w, h)
        for rho in (-1.0, 0.3, 1.0):
            X, Y = R.positions(M, w, h, rho)
            px, py = R.model_positions(M, w, h, rho)
            assert np.abs(X / 32.0 - px).max() <= 17.0 / 1024 + 1e-6
            assert np.abs(Y / 32.0 - py).max() <= 17.0 / 1024 + 1e-6
            assert np.abs(px - np.arange(w)[None, :]).max() > 0.5      # a real displacement


DIRECTION = [((6.0, 0.0, 0.0), 0.8), ((0.0, 5.0, 0.0), 0.8), ((4.0, -3.0, 0.01), 1.0), ((8.0, 2.0, 0.0), -0.5)]


def direction_errors(correct, seeds=(1, 2, 3), w=96, h=64, rim=8):
    """[(raw, with the true motion, with rho negated)]: mean absolute error against the global-shutter render, `rim` pixels in.
    correct(frame (h, w, 3) uint8, transform tuple, rho) -> the corrected frame"""
    out = []
    for motion, rho in DIRECTION:
        for seed in seeds:
            tex = R.binomial_noise(np.random.default_rng(seed), w, h)
            gs, rs, tr = R.shutter_renders(tex, w, h, motion, rho)
            err = lambda a: float(np.abs(a[rim:h - rim, rim:w - rim].astype(np.float64) - gs[rim:h - rim, rim:w - rim]).mean())
            out.append((err(rs), err(correct(rs, tr, rho)), err(correct(rs, tr, -rho))))
    return out


def test_direction_on_the_restatement(oracle):
    O = oracle
    errs = direction_errors(lambda f, tr, rho: R.rolling_frame(f, O.cv_inverse_matrix(O.Transform.of(*tr), f.shape[1], f.shape[0]), rho, 255))
    for raw, right, wrong in errs:
        print("raw %.3f  corrected %.3f (%.2f)  rho negated %.3f (%.2f)" % (raw, right, right / raw, wrong, wrong / raw))
    for raw, right, wrong in errs:
        assert raw > 1.0                                             # the shutter did distort the frame
        assert right < 0.5 * raw
        assert wrong > raw
