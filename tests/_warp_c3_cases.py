"""Inputs for the hostile tests of the float-tile warps -- VS_WARP_LANCZOS2, VS_WARP_BILINEAR, VS_WARP_LANCZOS2_FAST, VS_WARP_LANCZOS2_SEP, all of
them vs_k_bgr_warp_c3 (tests/test_c3_window_cpp.py, tests/test_warp_c3_hostile_gpu.py) -- and a numpy restatement of the tile-window decision
they share (video_stabilizer_amd/csrc/vs_c3_window.hpp), which tests/test_c3_window_cpp.py holds against the real function's decisions, so that
the premises asserted here are premises about the code that runs.  Like tests/_hostile_maps.py every builder ASSERTS ITS PREMISE on the CPU
before anything is handed to a kernel: where a premise fails, the input has to change, not the assertion.

Transforms are (A, B, TX, TY) tuples: the matrix is [[1 + A, -B], [B, 1 + A]] about the frame's centre plus the shift."""
import math

import numpy as np

import _hostile_maps as HM

F = np.float32
TILE_W = 64
# every instantiation of vs_k_bgr_warp_c3: (name, tile height, staged rows, column groups, row pitch in staged pixels, org, bytes per staged pixel)
SHAPES = [("standard_24x20x81", 16, 24, 20, 81, 1, 16), ("six_wave_20x20x81", 16, 20, 20, 81, 1, 16), ("seven_wave_20x18x73", 16, 20, 18, 73, 1, 16),
          ("raw_u8_40x20x88", 32, 40, 20, 88, 0, 4), ("raw_u16_24x20x88", 16, 24, 20, 88, 0, 8)]
STANDARD, SIX_WAVE, SEVEN_WAVE, RAW_U8, RAW_U16 = range(5)
MODES = {"lanczos2": 0, "bilinear": 1, "fast": 2, "sep": 3}          # VS_WARP_LANCZOS2, _BILINEAR, _LANCZOS2_FAST, _LANCZOS2_SEP = the oracle's twins
K_PARAM_SLOTS, K_TABLE_INTS = 1 << 15, 8 << 20                       # vs_call_plan.hpp: the parameter ring's float4 slots, the table ring's ints
MAX_EXTENT_FRAMES = K_PARAM_SLOTS // 2 // 2                          # vs_capi_warp.hip: with_extents needs 2 n <= kParamSlots / 2


# ---- the decision, restated -------------------------------------------------------------------------------------------------------------------
def params(t, w, h):
    """vs_ul_params_warp: the kernel's {A, B, TX, TY} about the upper left corner, rounded to float once"""
    A, B, TX, TY = (float(v) for v in t)
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    with np.errstate(all="ignore"):
        return np.array([A, B, TX - A * cx + B * cy, TY - B * cx - A * cy], np.float64).astype(F)


def extents(P, roi, tile_h):
    """vsd::c3_extents for one frame -> four floats, rounded outward"""
    A1, B, TX, TY = float(F(1) + P[0]), float(P[1]), float(P[2]), float(P[3])
    x, y, rw, rh = roi
    X, Y = float(x + rw) + 64.0, float(y + rh) + float(tile_h)
    M = max(abs(A1) * X + abs(B) * Y + abs(TX), abs(B) * X + abs(A1) * Y + abs(TY)) + 1.0
    eps = M * (1.0 / 1048576.0)
    ax, bx, ay, by = A1 * (TILE_W - 1), -B * (tile_h - 1), B * (TILE_W - 1), A1 * (tile_h - 1)
    v = [min(0.0, ax) + min(0.0, bx) - eps, max(0.0, ax) + max(0.0, bx) + eps, min(0.0, ay) + min(0.0, by) - eps, max(0.0, ay) + max(0.0, by) + eps]
    out = np.empty(4, F)
    for k in range(4):
        with np.errstate(all="ignore"):
            q = F(v[k])
        if not math.isfinite(v[k]) or not np.isfinite(q):
            q = F(3.0e38) if k & 1 else F(-3.0e38)
        elif (float(q) < v[k]) if k & 1 else (float(q) > v[k]):
            q = np.nextafter(q, F(np.inf) if k & 1 else F(-np.inf))
        out[k] = q
    return out


def compact_shape(E4):
    """vsd::c3_compact_shape over the frames' extents (n x 4)"""
    shape = 2
    for E in np.asarray(E4, F).reshape(-1, 4):
        if not float(E[3]) - float(E[2]) < 15.999:
            return 0
        if not float(E[1]) - float(E[0]) < 64.99:
            shape = 1
    return shape


def tile_window(P, roi, x0, y0, shape, E=None):
    """vsd::c3_tile_window for finite parameters: every product and sum in float32, in the function's order -> (fits, sx_lo, sy_lo, rows, groups)"""
    _, tile_h, max_rows, max_groups, pitch, org, _ = SHAPES[shape]
    A1, B, TX, TY = F(1) + P[0], P[1], P[2], P[3]
    x, y, rw, rh = roi
    fx0, fy0 = F(x0 + x), F(y0 + y)
    with np.errstate(all="ignore"):
        if E is not None:
            Wx00, Wy00 = A1 * fx0 - B * fy0 + TX, B * fx0 + A1 * fy0 + TY
            mnx, mxx, mny, mxy = Wx00 + E[0], Wx00 + E[1], Wy00 + E[2], Wy00 + E[3]
        else:
            fx1, fy1 = F(min(x0 + TILE_W, rw) - 1 + x), F(min(y0 + tile_h, rh) - 1 + y)
            xa, xb = (fx0, fx1) if A1 >= 0 else (fx1, fx0)
            ya, yb = (fy0, fy1) if B >= 0 else (fy1, fy0)
            mnx, mxx = A1 * xa - B * yb + TX, A1 * xb - B * ya + TX
            xc, xd = (fx0, fx1) if B >= 0 else (fx1, fx0)
            yc, yd = (fy0, fy1) if A1 >= 0 else (fy1, fy0)
            mny, mxy = B * xc + A1 * yc + TY, B * xd + A1 * yd + TY
    v = [mnx, mxx, mny, mxy]
    assert all(np.isfinite(q) or np.isinf(q) for q in v), "the restatement is for maps without NaN positions"
    if not max(abs(float(q)) for q in v) < 1.0e6:
        return (0, 0, 0, 0, 0)
    sx_lo = (int(math.floor(mnx)) - 1) & ~3
    sx_hi = int(math.floor(mxx)) + 2
    sy_lo = int(math.floor(mny)) - 1
    sy_hi = int(math.floor(mxy)) + 2
    rows, groups = sy_hi - sy_lo + 1, (sx_hi - sx_lo + 4) >> 2
    lim = (1 << 24) - pitch
    R = (sy_lo + org) * pitch
    I = R + sx_lo + org
    fits = groups <= max_groups and rows <= max_rows and abs(R) <= lim and abs(I) <= lim
    return (int(fits), sx_lo, sy_lo, rows, groups)


def decisions(t, w, h, roi, shape, with_extents):
    """the call's extents, what c3_compact_shape makes of them, and every tile's decision in raster order (x0, y0, fits, sx_lo, sy_lo, rows, groups)"""
    P = params(t, w, h)
    tile_h = SHAPES[shape][1]
    E = extents(P, roi, tile_h)
    tiles = [(x0, y0) + tile_window(P, roi, x0, y0, shape, E if with_extents else None) for y0 in range(0, roi[3], tile_h) for x0 in range(0, roi[2], TILE_W)]
    return E, compact_shape(E), np.array(tiles, np.int64).reshape(-1, 7)


def positions(t, w, h):
    """the sampling positions of every frame pixel as the kernels form them (float32, the reference's order of operations)"""
    P = params(t, w, h)
    A1, B, TX, TY = F(1) + P[0], P[1], P[2], P[3]
    fx, fy = np.arange(w, dtype=F)[None, :], np.arange(h, dtype=F)[:, None]
    with np.errstate(all="ignore"):
        return A1 * fx - B * fy + TX, B * fx + A1 * fy + TY


def launched_shape(mode, bits, ts, w, h, roi, n_frames=None):
    """the instantiation that vs_capi_warp.hip / vsk::bgr_warp_c3 launch for this call, an index into SHAPES"""
    if mode == MODES["bilinear"]:
        return RAW_U8 if bits == 8 else RAW_U16
    n = len(ts) if n_frames is None else n_frames
    if mode == MODES["lanczos2"] or n > MAX_EXTENT_FRAMES:
        return STANDARD
    c = compact_shape(np.stack([extents(params(t, w, h), roi, 16) for t in ts]))
    return STANDARD if c == 0 else (SEVEN_WAVE if c == 2 and mode == MODES["sep"] else SIX_WAVE)


def table_ints(roi_w, roi_h):
    """vs_warp_table.hpp: ints of table per frame -- one 16-byte entry per 64 x 16 tile, one 8-byte pair per row of the run padded to 4-row blocks"""
    tiles = -(-roi_w // 64) * -(-roi_h // 16)
    return (16 * tiles + 8 * (-(-roi_h // 4) * 4)) // 4


def tables_fit(n, roi_w, roi_h):
    """vs_call_plan.hpp: plan::aligned_tables_fit -- the take (3 ints of alignment slack) stays within half the table ring"""
    return table_ints(roi_w, roi_h) * n + 3 <= K_TABLE_INTS // 2


# ---- maps ---------------------------------------------------------------------------------------------------------------------------------------
ROW_LIMIT = {pitch: (1 << 24) / pitch for pitch in (73, 81, 88)}      # source rows from which (sy_lo + org) pitch leaves fp32's exact integers
FAR = (1e4, 1.9e5, 1.95e5, 2.05e5, 2.1e5, 2.25e5, 2.35e5, 3e5, 9.9e5, 999900.0, 1000100.0)
assert 1.9e5 < ROW_LIMIT[88] < 1.95e5 and 2.05e5 < ROW_LIMIT[81] < 2.1e5 and 2.25e5 < ROW_LIMIT[73] < 2.35e5


def far_shifts():
    """{name: transform}: identity scale with the shifts of FAR in +-x, +-y and both (the fractions .3 / .25 keep every tap weighted), and a half
    degree turn at the far rows"""
    out = {}
    for s in FAR:
        for sg, sn in ((1, "p"), (-1, "m")):
            v = sg * (s + 0.25)
            out["far_x_%s%g" % (sn, s)] = (0.0, 0.0, v, -0.45)
            out["far_y_%s%g" % (sn, s)] = (0.0, 0.0, 0.3, v)
            out["far_xy_%s%g" % (sn, s)] = (0.0, 0.0, -v, v)
    a = math.radians(0.5)
    for s in (2.1e5, 2.35e5, 3e5):
        out["far_y_turn_p%g" % s] = (math.cos(a) - 1, math.sin(a), 0.3, s + 0.25)
        out["far_y_turn_m%g" % s] = (math.cos(a) - 1, -math.sin(a), 0.3, -s - 0.25)
    return out


def far_rows():
    """the far-row maps by name: rows beyond every pitch's exactness limit in +y and -y, columns inside the frame"""
    return {k: v for k, v in far_shifts().items() if k.startswith("far_y_") and "turn" not in k and ROW_LIMIT[88] < abs(v[3]) < 9.99e5}


def hostile_maps(w, h):
    """{name: transform}: the maps of HM.HOSTILE and HM.FILL_EXTREME whose float32 positions over the frame are finite and below 2^30 (the
    others stay with test_non_finite_transforms_stay_inside_their_buffers), and the far shifts.  Premises asserted: the positions, and that the
    far rows lie beyond each pitch's limit"""
    maps = {}
    for k, t in list(HM.HOSTILE.items()) + list(HM.FILL_EXTREME.items()):
        Wx, Wy = positions(t, w, h)
        if np.isfinite(Wx).all() and np.isfinite(Wy).all() and max(np.abs(Wx).max(), np.abs(Wy).max()) < 2.0 ** 30:
            maps[k] = t
    assert len(maps) == 19 and "tx_m3e6" in maps and "p1e300" not in maps and not set(maps) & set(HM.HAS_NAN), sorted(maps)
    maps.update(far_shifts())
    for k, t in far_rows().items():
        Wx, Wy = positions(t, w, h)
        assert Wx.min() > 0 and Wx.max() < w and np.abs(Wy).min() > ROW_LIMIT[88]
    assert any(abs(t[3]) > ROW_LIMIT[73] for t in far_rows().values())
    return maps


def WINDOWS(w, h):
    """the output windows of part 1, those the frame holds: whole, one-row, narrow, from the second tile on, one-column, inner at odd offsets, the
    last pixel, and 17 / 33 rows -- a last tile row with one live row for the 16- / 32-row tiles"""
    full = [(0, 0, w, h), (0, 0, w, 1), (3, 0, 33, 1), (64, 0, w - 64, 1), (0, h - 1, w, 1), (0, 0, 1, h), (5, 7, 21, 11), (w - 1, h - 1, 1, 1),
            (0, 0, w, 17), (1, 3, w - 1, 33)]
    out = []
    for x, y, rw, rh in full:
        if rw >= 1 and rh >= 1 and x >= 0 and y >= 0 and x + rw <= w and y + rh <= h and (x, y, rw, rh) not in out:
            out.append((x, y, rw, rh))
    return out


def _turn(deg, zoom, tx, ty):
    a = math.radians(deg)
    return (zoom * math.cos(a) - 1.0, zoom * math.sin(a), tx, ty)


SWEEP_SHAPE = (130, 70)
SWEEP_WINDOWS = [(0, 0, 130, 70), (3, 5, 125, 8)]                     # full tiles; 8 rows, where the column groups bind before the rows


def fit_sweep():
    """[(name, transform)]: zooms 1.00 .. 1.40 (a 64 x 16 tile reads 64 z columns and 16 z rows: 18 groups are passed near 1.03, 20 near 1.16,
    20 rows near 1.0, 24 near 1.25, the 8-bit raw tile's 40 for 32 near 1.13), alone and turned by 0.6 and -2.5 degrees, with sub-pixel shifts;
    then maps on both sides of c3_compact_shape's thresholds (15.999 rows: a zoom of 1.0666 less eps; 64.99 columns: 1.03159).
    The premises -- footprints at each shape's rows / groups and one beyond, the thresholds' sides -- are asserted by sweep_premises"""
    out = []
    for i, z in enumerate(np.arange(1.0, 1.4001, 0.0125)):
        for deg in (0.0, 0.6, -2.5):
            sh = ((0.0, 0.0), (0.3, 0.6), (-0.45, 0.2))[i % 3]
            out.append(("zoom%.4f_turn%+.1f" % (z, deg), _turn(deg, float(z), sh[0], sh[1])))
    return out + THRESHOLD_MAPS


# (name, transform, the launcher's shape for the frame alone on SWEEP_SHAPE's whole window)
_THRESHOLDS = [("rows_below", _turn(0.0, 1.0660, 0.3, 0.6), 1), ("rows_above", _turn(0.0, 1.0670, 0.3, 0.6), 0),
               ("cols_below", _turn(0.0, 1.0310, -0.45, 0.2), 2), ("cols_above", _turn(0.0, 1.0320, -0.45, 0.2), 1),
               ("turn_rows_below", _turn(0.85, 1.0, 0.0, 0.0), 2), ("turn_rows_above", _turn(0.95, 1.0, 0.0, 0.0), 0)]
THRESHOLD_MAPS = [(n, t) for n, t, _ in _THRESHOLDS]
# batches that mix sides: the launcher must fall back for all frames
MIXED_BATCHES = {"seven_and_six": (["cols_below", "cols_above", "cols_below"], 1), "six_and_standard": (["rows_below", "rows_above"], 0),
                 "seven_and_standard": (["turn_rows_below", "cols_below", "turn_rows_above"], 0), "all_seven": (["cols_below", "turn_rows_below"], 2)}


def sweep_premises():
    """asserts what the sweep is for, with the restated decision: per instantiation, on SWEEP_SHAPE's windows, tiles whose footprint has exactly
    max_rows rows, max_rows + 1, max_groups groups and max_groups + 1 (with and without extents taken together); each threshold map's shape;
    each mixed batch's shape"""
    w, h = SWEEP_SHAPE
    seen = {k: set() for k in range(len(SHAPES))}
    for _, t in fit_sweep():
        for roi in SWEEP_WINDOWS:
            for k in range(len(SHAPES)):
                for we in (False, True):
                    d = decisions(t, w, h, roi, k, we)[2]
                    seen[k] |= {("rows", int(r)) for r in d[:, 5]} | {("groups", int(g)) for g in d[:, 6]}
    for k, (name, _, max_rows, max_groups, _, _, _) in enumerate(SHAPES):
        for want in (("rows", max_rows), ("rows", max_rows + 1), ("groups", max_groups), ("groups", max_groups + 1)):
            assert want in seen[k], (name, want, sorted(seen[k]))
    by_name = dict(THRESHOLD_MAPS)
    for name, t, shape in _THRESHOLDS:
        assert compact_shape(extents(params(t, w, h), (0, 0, w, h), 16)) == shape, name
    for name, (names, shape) in MIXED_BATCHES.items():
        E = np.stack([extents(params(by_name[n], w, h), (0, 0, w, h), 16) for n in names])
        assert compact_shape(E) == shape, name
        assert len({compact_shape(e) for e in E}) > 1 or name == "all_seven", name
