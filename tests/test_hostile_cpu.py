"""-m "not gpu": the premises and the references of the hostile tests (tests/_hostile_maps.py), before a kernel is involved.

  * the fill's coverage rule in its two forms (tests/_fill_ref.py): int32 with saturation and wrap -- the rule, what the oracle's plain warp
    does -- against unbounded int64; where they part and where they agree;
  * the deblur rule's restatement (tests/_deblur_ref.py) against the rule written directly in float64 (tests/_deblur_direct.py);
  * the parameter boundary of vs_deblur_params on the restatement;
  * every premise of the GPU cases (the builders assert them)."""
import numpy as np
import pytest

import _deblur_direct as D
import _deblur_ref as R
import _fill_ref as RF
import _hostile_maps as HM


def test_int32_coverage_is_the_plain_warp_and_int64_is_not(oracle):
    """the transforms of the finding: near-singular, rotated.  The int64 form covers nothing; the int32 form covers exactly the pixels at
    which the oracle's plain warp of an all-max frame returns max (all four taps inside: no border value mixed in)"""
    O = oracle
    w, h = 64, 48
    n = 0
    for name in HM.NEAR_SINGULAR:
        t = O.Transform.of(*HM.FILL_EXTREME[name])
        a, b = RF.covered(O, t, w, h), RF.covered_int64(O, t, w, h)
        assert not np.array_equal(a, b) and not b.any() and a.sum() > 2000, (name, int(a.sum()), int(b.sum()))
        for dtype, maxv in ((np.uint8, 255), (np.uint16, 1023)):
            full = O.bgr_image_warp(np.full((h, w, 3), maxv, dtype), t, O.WARP_BILINEAR_CV, border=O.BORDER_CONSTANT, max_value=maxv)
            assert np.array_equal(a, (full == maxv).all(-1)), name
        n += 1
    assert n == 6
    # the large translations: both forms cover nothing, for different reasons
    for name in ("tx_6e5", "ty_m6e5", "tx_m3e6", "ty_3e6", "t_1e300"):
        t = O.Transform.of(*HM.FILL_EXTREME[name])
        assert not RF.covered(O, t, w, h).any() and not RF.covered_int64(O, t, w, h).any(), name


def test_the_two_coverage_forms_agree_on_every_transform_the_other_tests_draw(oracle):
    import test_fill_gpu as TG
    O = oracle
    n = 0
    for bits in (8, 10):
        for n_cand in (1, 2, 5, 16):
            _, ct = TG._cands(O, np.random.default_rng(100 * bits + n_cand), 5, n_cand, 6, 203, 149)
            ct[3][0] = O.Transform.of(0.0, 0.0, 5000.0, -3000.0)
            for t in (t for row in ct for t in row):
                assert np.array_equal(RF.covered(O, t, 203, 149), RF.covered_int64(O, t, 203, 149))
                n += 1
    for tr in [(0.01, -0.02, 7.3, -4.6), (-0.03, 0.015, -11.2, 6.1), (0, 0, 0.5, 0.5), (0.2, 0.1, 30.0, 20.0), (0, 0, 500.0, 0), (0.004, -0.006, 23.5, -17.25)]:
        for w, h in ((131, 77), (90, 120), (1920, 1080)):
            assert np.array_equal(RF.covered(O, O.Transform.of(*tr), w, h), RF.covered_int64(O, O.Transform.of(*tr), w, h))
            n += 1
    assert n > 100


def test_premises_of_the_tie_and_trap_cases(vs):
    for w, h in HM.DEBLUR_SHAPES + [(64, 48), (63, 47), (12, 9)]:
        assert len(HM.tie_maps(vs, w, h)) == 6
    for w, h in ((64, 48), (300, 270)):
        HM.row0_trap(vs, w, h)
    for name in HM.HAS_NAN:
        assert np.isnan(np.asarray(HM.cvinv(vs)(vs.Transform.of(*HM.HOSTILE[name]), 64, 48))).any(), name
    assert not np.asarray(HM.cvinv(vs)(vs.Transform.of(*HM.HOSTILE["singular"]), 64, 48)).any()
    assert np.abs(np.asarray(HM.cvinv(vs)(vs.Transform.of(*HM.HOSTILE["near_pp"]), 64, 48))).min() > 1e8


# share of samples at which round(direct) and the restatement differ, measured when this was written (two CPU programs: the same on every
# machine), and the gate: twice that, rounded up to one significant digit
DIRECT_SHARE = {"bgr8": 2.82e-4, "bgr10": 3.88e-4, "bgr12": 3.55e-4, "bgr16": 1.10e-3}
DIRECT_SHARE_GATE = {"bgr8": 6e-4, "bgr10": 8e-4, "bgr12": 8e-4, "bgr16": 3e-3}


@pytest.mark.parametrize("fmt", sorted(HM.FORMATS))
def test_restatement_against_the_direct_form(vs, fmt):
    """part A's shapes with well-conditioned maps (no ties, no out-of-range samples: there the nearest pixel and the clamp are rules, not
    values).  round(direct) and the restatement differ by at most 1 LSB, and only where the float64 quotient lies within the fp32 error
    bound of a .5 boundary (tests/_deblur_direct.py derives it: 43 roundings, 48 u (q + 1) asserted).  Share of differing samples when
    this was written: 2.82e-4 (bgr8), 3.88e-4 (bgr10), 3.55e-4 (bgr12), 1.10e-3 (bgr16) of 685 272 samples each (DIRECT_SHARE); asserted with
    a margin of twice that, rounded up to one digit (DIRECT_SHARE_GATE)."""
    code, dtype, bits = HM.FORMATS[fmt]
    maxv = (1 << bits) - 1
    differ = total = 0
    for w, h in HM.DEBLUR_SHAPES:
        src, S, cf, maps = HM.deblur_case(vs, fmt, w, h, direct=True)
        ct = HM.transforms(vs, maps)
        for o in range(len(cf)):
            want = R.deblur_frame(HM.cvinv(vs), src, S, list(cf[o]), ct[o], bits, maxv)
            quot = D.deblur_frame(src, S, list(cf[o]), ct[o], bits)
            nd, bad = D.compare(quot, want, maxv)
            assert bad == 0, (w, h, o, nd, bad)
            differ += nd
            total += want.size
    print("%s: %d of %d samples differ between round(direct) and the restatement (share %.3g)" % (fmt, differ, total, differ / total))
    assert differ <= DIRECT_SHARE_GATE[fmt] * total


def test_parameter_boundary_on_the_restatement(vs):
    """the black target and the two saturated 16-bit candidates of the finding.  Just inside include/vs_amd.h's condition W is finite (and
    reaches 2^99: the boundary is the one that matters); outside it, at the old box's corners, W is inf and acc / W is inf / inf"""
    src, S = HM.black_target_stack(np.random.default_rng(3))
    S = HM.BIG_S                                                     # (the call takes S from the caller: ratios up to 2^53)
    cf, ct = [0, 1, 2], [vs.Transform.of()] * 3
    for sens, mr in ((2.0, 4.0), (0.5, 1.75), (8.0, 100.0)):
        assert HM.params_accepted(sens, mr)
    inside = [(2.0 ** -96, 4.0), (1.0, 2.0 ** 50), (2.0 ** 6, 1.0e18), (2.0 ** 6, 2.0 ** 53)]
    for sens, mr in inside:
        assert HM.params_accepted(sens, mr), (sens, mr)
        with np.errstate(all="raise"):
            out, W, raw = R.deblur_frame(HM.cvinv(vs), src, S, cf, ct, 16, 65535, sens, mr, want_raw=True)
        assert np.isfinite(W).all() and np.isfinite(raw).all() and W.max() >= 2.0 ** 99, (sens, mr, W.max())
    for sens, mr in ((float(np.nextafter(np.float32(2.0 ** -96), np.float32(0))), 4.0), (1.0, float(np.nextafter(np.float32(2.0 ** 50), np.float32(np.inf)))),
                     (float(np.nextafter(np.float32(2.0 ** 6), np.float32(0))), 1.0e18), (1e-30, 1e18), (1e-38, 4.0)):
        assert not HM.params_accepted(sens, mr), (sens, mr)
    for sens, mr in ((1e-30, 1e18), (1e-38, 4.0)):                   # what the old box let through
        with np.errstate(all="ignore"):
            out, W, raw = R.deblur_frame(HM.cvinv(vs), src, S, cf, ct, 16, 65535, sens, mr, want_raw=True)
        assert np.isinf(W).any() and np.isnan(raw).any(), (sens, mr)
