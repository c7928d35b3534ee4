"""Inputs for the hostile tests of the deblur and the border fill (tests/test_deblur_hostile_gpu.py, tests/test_fill_hostile_gpu.py,
tests/test_hostile_cpu.py): transforms at the edges of what the C ABI accepts, and content that makes the rule's clamps live.  Every
builder ASSERTS ITS PREMISE on the CPU references alone -- the property that makes the input hostile -- before anything is handed to a
kernel (tests/_flow_cases.py does the same for the dense flow): where a premise fails, the input has to change, not the assertion.

Transforms are (A, B, TX, TY) tuples: the matrix is [[1 + A, -B], [B, 1 + A]] about the frame's centre plus the shift."""
import numpy as np

import _deblur_ref as R

NAN, INF = float("nan"), float("inf")
FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}

# maps whose handling the code specifies and no moderate input reaches
HOSTILE = {
    "nan_A": (NAN, 0.0, 0.0, 0.0), "nan_B": (0.0, NAN, 0.0, 0.0), "nan_TX": (0.0, 0.0, NAN, 0.0), "nan_TY": (0.01, -0.02, 1.0, NAN),
    "inf_TX": (0.0, 0.0, INF, 0.0), "ninf_TY": (0.0, 0.0, 0.0, -INF), "inf_both": (0.01, 0.02, -INF, INF),
    "p1e300": (0.0, 0.0, 1e300, 1e300), "m1e300": (0.01, -0.02, -1e300, 1e300),
    "singular": (-1.0, 0.0, 0.0, 0.0),
    "near_pp": (-1 + 1e-9, 1e-9, 3.0, 2.0), "near_pm": (-1 + 1e-9, -1e-9, 0.0, 0.0),
    "near_mp": (-1 - 1e-9, 1e-9, 0.0, 0.0), "near_mm": (-1 - 1e-9, -1e-9, 3.0, 2.0),
    "rot90_zoom05": (-1.0, 0.5, 0.0, 0.0), "rot90_zoom2": (-1.0, 2.0, 1.0, -1.0),
    "rot180_zoom05": (-1.5, 0.0, 0.5, 0.0), "rot180_zoom2": (-3.0, 0.0, -2.0, 1.0),
}
HAS_NAN = ("nan_A", "nan_B", "nan_TX", "nan_TY", "inf_TX", "ninf_TY", "inf_both")      # (an infinite shift: -inf and inf - inf in the inverse)
# the near-singular rotated transforms on which int64 and int32 coverage part (tests/test_fill_cpu.py), and large translations: beyond the
# fill's 2^29 table-term guard (6e5 px), beyond cvRound's saturation (3e6 px), beyond everything (1e300)
FILL_EXTREME = {
    "near_pp0": (-1 + 1e-9, 1e-9, 0.0, 0.0), "near_pn0": (-1 + 1e-9, -1e-9, 0.0, 0.0), "near_pp_shift": (-1 + 1e-9, 1e-9, 3.0, 2.0),
    "near_1e-8": (-1 + 1e-8, 1e-8, 0.0, 0.0), "near_1e-7": (-1 + 1e-7, -1e-7, 0.0, 0.0), "near_1e-6": (-1 + 1e-6, 1e-6, 0.0, 0.0),
    "tx_6e5": (0.0, 0.0, 6e5, 0.0), "ty_m6e5": (0.0, 0.0, 0.0, -6e5), "tx_m3e6": (0.0, 0.0, -3e6, 3e6), "ty_3e6": (0.01, 0.0, 0.0, 3e6),
    "t_1e300": (0.0, 0.0, 1e300, -1e300),
}
NEAR_SINGULAR = ("near_pp0", "near_pn0", "near_pp_shift", "near_1e-8", "near_1e-7", "near_1e-6")

# shapes of part A: tiny and one-sided; across the per-sample kernel's 64 x 64 tile; across the x4 kernel's 256 x 64 tile (widths that are
# multiples of 4)
DEBLUR_SHAPES = [(1, 1), (1, 5), (3, 1), (2, 2), (4, 1), (4, 17), (8, 16), (63, 15), (65, 65), (67, 129), (64, 16), (256, 64), (260, 65), (516, 17)]


def T(mod, tup):
    return mod.Transform.of(*tup)


def cvinv(vs):
    def f(t, w, h):
        with np.errstate(all="ignore"):
            return vs.cv_inverse_matrix(vs.Transform.of(*t.tup()), w, h)
    return f


def contrast_stack(rng, n, w, h, dtype, maxv):
    """n frames of independent noise at contrasts 1/n .. 1: frame i + 1 is sharper than frame i wherever a frame has an interior"""
    out = []
    for i in range(n):
        noise = rng.integers(0, maxv + 1, (h, w, 3)).astype(np.float64)
        out.append(np.clip(np.floor(maxv / 2 + (noise - maxv / 2) * (i + 1) / n), 0, maxv))
    return np.stack(out).astype(dtype)


# ---- rint ties ---------------------------------------------------------------------------------------------------------------------------
def tie_share(M, w, h):
    """share of the pixels at which ties-to-even and round-half-up name different samples"""
    M = np.asarray(M, np.float64).reshape(6)
    xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    vx, vy = (M[0] * xs + M[1] * ys) + M[2], (M[3] * xs + M[4] * ys) + M[5]
    return float(((np.rint(vx) != np.floor(vx + 0.5)) | (np.rint(vy) != np.floor(vy + 0.5))).mean()), vx, vy


TIE_TRANSLATIONS = [(0.0, 0.0, 0.5, 0.5), (0.0, 0.0, -0.5, 1.5), (0.0, 0.0, 2.5, -0.5), (0.0, 0.0, 0.5, 0.0), (0.0, 0.0, 0.0, -1.5)]


def tie_maps(vs, w, h):
    """[(name, transform tuple)] whose maps put EVERY pixel on a tie in x, in y or in both: half-integer translations, and the 45 degree
    rotation with zoom 1 / sqrt 2 (1 + A = B = 0.5: every entry of the inverse is +-1 exactly) shifted so that M2 and M5 are k + 0.5 --
    a rotated map on which whole columns and rows of (M0 x + M1 y) + M2 are exactly representable.  Premises asserted: more than half of
    the pixels differ between rint and floor(v + 0.5) for the maps that tie on both axes (more than a fifth for the one-axis ones), and the
    positions -0.5, w - 1.5 and w - 0.5 (likewise in y) occur in front of the rounding"""
    out = []
    seen_x, seen_y = set(), set()
    for tr in TIE_TRANSLATIONS:
        M = cvinv(vs)(vs.Transform.of(*tr), w, h)
        share, vx, vy = tie_share(M, w, h)
        both = tr[2] % 1 != 0 and tr[3] % 1 != 0
        if w >= 4 and h >= 4:
            assert share > (0.5 if both else 0.2), (tr, w, h, share)
        seen_x |= set(np.unique(vx)) & {-0.5, w - 1.5, w - 0.5}
        seen_y |= set(np.unique(vy)) & {-0.5, h - 1.5, h - 0.5}
        out.append(("shift_%g_%g" % tr[2:], tr))
    assert seen_x == {-0.5, w - 1.5, w - 0.5} and seen_y == {-0.5, h - 1.5, h - 0.5}, (w, h, seen_x, seen_y)
    # the rotated one: x' = c + T + R (x - c) with R = [[.5, -.5], [.5, .5]]; the inverse's translation is made k + 0.5 by the shift
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    for tx, ty in ((0.25 * i, 0.25 * j) for i in range(8) for j in range(8)):
        tr = (-0.5, 0.5, tx, ty)
        M = np.asarray(cvinv(vs)(vs.Transform.of(*tr), w, h), np.float64)
        share, _, _ = tie_share(M, w, h)
        # (x + y and x - y have the same parity: the two axes' ties are correlated, and only shifts whose integer parts differ in parity
        # put the share above one half -- at 1, in fact)
        if M[2] % 1 == 0.5 and M[5] % 1 == 0.5 and (share > 0.5 or w < 4 or h < 4):
            assert np.array_equal(np.abs(M[[0, 1, 3, 4]]), np.ones(4)), M
            out.append(("rot45_ties", tr))
            break
    else:
        raise AssertionError("no shift puts the rotated map on ties at %d x %d" % (w, h))
    return out


# ---- out-of-range samples ------------------------------------------------------------------------------------------------------------------
def out_of_range_stack(rng, n, w, h, bits):
    """10- / 12-bit containers that hold 65535 and max_value + 1 at scattered pixels of every frame.  Premise: the gray before its clamp
    exceeds 255 somewhere in every frame"""
    maxv = (1 << bits) - 1
    src = contrast_stack(rng, n, w, h, np.uint16, maxv)
    for f in src:
        m = rng.random((h, w)) < 0.08
        f[m] = 65535
        m = rng.random((h, w, 3)) < 0.05
        f[m] = maxv + 1
        f[0, 0] = 65535                                              # (tiny frames: at least one)
        assert R.gray_unclamped(f, bits).max() > 255
    return src


# ---- the parameter boundary ---------------------------------------------------------------------------------------------------------------
def params_accepted(sensitivity, max_ratio):
    """include/vs_amd.h's condition on vs_deblur_params, restated"""
    s, m = float(np.float32(sensitivity)), float(np.float32(max_ratio))
    return 0 < s <= 3.0e38 and 0 < m <= 1.0e18 and min(m, 2.0 ** 53) ** 2 <= s * 2.0 ** 100


BIG_S = np.array([0, 1 << 52, (1 << 53) - 1], np.uint64)             # the largest sharpness the rule allows (S < 2^53) over a black target


def black_target_stack(rng, w=16, h=16):
    """a black target (S_k = 0) and two 16-bit candidates of 0 / 65535 noise: with d = 0 wherever a candidate is black too, the weights are
    max_ratio^2 / sensitivity exactly -- the input on which the old parameter box overflowed the fp32 sums"""
    src = np.zeros((3, h, w, 3), np.uint16)
    src[1:] = (rng.integers(0, 2, (2, h, w, 1)) * 65535).astype(np.uint16)
    # some dark but non-black candidate samples whose gray is 0 (d = 0): the largest weights meet non-zero samples
    src[1, ::3, ::2] = (1000, 50, 20)
    src[2, 1::3, ::2] = (900, 40, 100)
    S = R.sharpness_batch(src, 16)
    assert S[0] == 0 and S[1] > 0 and S[2] > 0
    assert (R.gray8(src[1, ::3, ::2], 16) == 0).all() and (R.gray8(src[2, 1::3, ::2], 16) == 0).all()
    return src, S


def row0_trap(vs, w, h):
    """a near-singular transform (A = -1 - 1e-9, B = 1e-9: M0 = M3 = M4 = -5e8) shifted so that M2 = -0.5 and M5 = -0.25: on frame row 0 the
    row origins are small and negative while adelta and bdelta saturate to INT_MIN from x = 1 on.  Nothing of row 0 is covered (x = 0 lies
    left of the frame, the others wrap to 2^21 px), yet all eight corner terms of a one-row rectangle there are below 2^29 in magnitude or
    are INT_MIN itself -- whose abs() is negative.  Premises asserted: the terms are what this says, and the rule covers nothing of row 0"""
    import _fill_ref as RF
    A, B = -1 - 1e-9, 1e-9
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    tul = -np.array([[1 + A, -B], [B, 1 + A]]) @ np.array([-0.5, -0.25])
    tr = (A, B, float(tul[0] + A * cx - B * cy), float(tul[1] + B * cx + A * cy))
    X0, Y0, ad, bd = RF._table_terms(vs, vs.Transform.of(*tr), w, h, RF.cv_round_sat)
    assert -1024 < X0[0, 0] < 0 and -1024 < Y0[0, 0] < 0 and ad[0, 0] == 0 and bd[0, 0] == 0
    assert (ad[0, 1:] == RF.INT32_MIN).all() and (bd[0, 1:] == RF.INT32_MIN).all()
    assert not RF.covered(vs, vs.Transform.of(*tr), w, h)[0].any()
    return tr


# ---- part A's input per shape ---------------------------------------------------------------------------------------------------------------
SYNTH_S = np.array([0, 1, 7, 7, 1000, 1 << 40], np.uint64)             # handed in as the frames' sharpness: S_k = 0, S_k = 1, a tie, a huge ratio


def _rot(rng, w, h, big=False):
    if big:                                                          # up to +-0.5 rad, zoom 0.6 .. 1.6
        z, a = rng.uniform(0.6, 1.6), rng.uniform(-0.5, 0.5)
        return (z * np.cos(a) - 1, z * np.sin(a), rng.uniform(-0.2, 0.2) * w, rng.uniform(-0.2, 0.2) * h)
    return (rng.uniform(-0.04, 0.04), rng.uniform(-0.05, 0.05), rng.uniform(-0.15, 0.15) * w, rng.uniform(-0.15, 0.15) * h)


def deblur_case(vs, fmt, w, h, direct=False):
    """-> (src, S, cand_frame, cand_t as tuples) for one shape and format: six noise frames, the sharpness of SYNTH_S (the call takes it from
    the caller: frames without an interior take part too), four output frames of five candidates.  Candidates: small and large rotations
    with zoom, tie translations, NaN / infinite / singular / near-singular / quarter-turn maps, a list cut by -1, a copy.
    direct=True: the variant for the comparison with tests/_deblur_direct.py -- well-conditioned random maps only (a tie's nearest pixel
    and a near-singular inverse are rules, not values)"""
    code, dtype, bits = FORMATS[fmt]
    rng = np.random.default_rng(1000 * w + 10 * h + bits)
    src = contrast_stack(rng, 6, w, h, dtype, (1 << bits) - 1)
    ident = (0.0, 0.0, 0.0, 0.0)
    if direct:
        maps = [[ident] + [_rot(rng, w, h, big=c % 2 == 1) for c in range(4)] for _ in range(4)]
        maps[3][2] = HOSTILE["p1e300"]
    else:
        ties = tie_maps(vs, w, h)
        maps = [[ident, _rot(rng, w, h), ties[(w + h) % 3][1], HOSTILE["nan_TX"], ties[-1][1]],
                [ident, ties[3][1], _rot(rng, w, h, big=True), ident, ties[1][1]],
                [ident] + [_rot(rng, w, h) for _ in range(4)],
                [ident, HOSTILE["rot90_zoom2"], HOSTILE["singular"], HOSTILE["near_pp"], _rot(rng, w, h, big=True)]]
    cf = np.array([[0, 4, 5, 2, 1], [2, 3, 4, -1, 5], [5, 4, 3, 2, 1], [1, 5, 4, 2, 3]], np.int32)
    return src, SYNTH_S, cf, maps


def transforms(mod, maps):
    return [[mod.Transform.of(*t) for t in row] for row in maps]
