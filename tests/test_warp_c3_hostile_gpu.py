"""The float-tile warps -- VS_WARP_LANCZOS2, VS_WARP_BILINEAR, VS_WARP_LANCZOS2_FAST, VS_WARP_LANCZOS2_SEP, all of them vs_k_bgr_warp_c3
(vs_warp.hip), the last two with the per-launch tables of vs_k_warp_c3_tables -- on hostile input: singular, near-singular, mirrored and
quarter-turn maps, shifts of 10^4 to beyond 10^6 pixels in x, in y and in both, FAR ROWS (columns inside the frame, rows beyond 2^24 / pitch,
where the sampler's fp32 tile offset is no longer exact and the window decision has to refuse the tile), one-row windows and tiles, maps at and
one beyond each instantiation's staged rows and column groups and on both sides of the launcher's two thresholds, batches that mix window
shapes, the three launch routes (tables, extents without tables, no extents), unaligned pitched device memory inside guard bands -- bit for
bit against the oracle's twin of the mode: the whole frame's oracle.bgr_image_warp, cut to the window.  Inputs and the restated window
decision: tests/_warp_c3_cases.py; the decision itself is held against the sampler's positions on the host (tests/test_c3_window_cpp.py),
where the form it replaced is shown to be inexact on the far rows.

Content: samples from max_value // 8 to max_value - max_value // 8, never 0, the frames of a batch distinct: a tile that read zeros (nothing
staged) cannot pass under VS_BORDER_CLAMP, and on the far rows a tap window one staged pixel off is a column shift of noise."""
import ctypes as C

import numpy as np
import pytest

import _warp_c3_cases as WC

pytestmark = pytest.mark.gpu

SHAPES = [(130, 70), (67, 21), (200, 1)]
FORMATS = {"bgr8": (np.uint8, 255), "bgr10": (np.uint16, 1023), "bgr16": (np.uint16, 65535)}      # name -> (dtype, max_value)
MODES = sorted(WC.MODES)                                              # the mode numbers are the C ABI's and the oracle's alike
BORDERS = (0, 1)                                                     # VS_BORDER_CLAMP, VS_BORDER_CONSTANT
G = 3

_cache = {}


def _content(fmt, n, w, h, seed=0):
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(1000 * w + 10 * h + maxv + seed)
    src = rng.integers(maxv // 8, maxv - maxv // 8 + 1, (n, h, w, 3)).astype(dtype)
    assert src.min() > 0 and len({f.tobytes() for f in src}) == n
    return src


def _twin(O, src, maps, mode, border, maxv):
    with np.errstate(all="ignore"):
        out = np.stack([O.bgr_image_warp(src[i], O.Transform.of(*t), WC.MODES[mode], border=border, max_value=maxv) for i, t in enumerate(maps)])
    out.setflags(write=False)
    return out


def _case(O, fmt, shape, mode):
    """-> names, transforms, frames (one per map) and {border: expected whole frames} of part 1 for one format, shape and mode; computed once"""
    key = (fmt, shape, mode)
    if key not in _cache:
        w, h = shape
        maps = WC.hostile_maps(w, h)
        names = sorted(maps)
        if ("src", fmt, shape) not in _cache:
            _cache[("src", fmt, shape)] = _content(fmt, len(names), w, h)
            _cache[("src", fmt, shape)].setflags(write=False)
        src = _cache[("src", fmt, shape)]
        want = {b: _twin(O, src, [maps[n] for n in names], mode, b, FORMATS[fmt][1]) for b in BORDERS}
        # under the clamp every expected sample is a weighted mean of frame samples, none of them 0: no expected frame has a tile of zeros (the
        # Lanczos2 forms' negative lobes can take a lone sample of noise down to 0, the bilinear mode nothing)
        assert all((f > 0).mean() > 0.99 for f in want[O.BORDER_CLAMP]) and (mode != "bilinear" or want[O.BORDER_CLAMP].min() > 0)
        _cache[key] = (names, [maps[n] for n in names], src, want)
    return _cache[key]


def _bad(names, got, want):
    return [n for i, n in enumerate(names) if not np.array_equal(got[i], want[i])]


def _far_row_premise(names, want_clamp, w):
    """the far-row frames under the clamp are the frame's first / last row, sampled at a fraction: noise, more than w / 2 distinct values in a
    row and none of them 0 -- a tap window one staged pixel off cannot go unseen"""
    far = [i for i, n in enumerate(names) if n in WC.far_rows()]
    assert len(far) >= 12
    for i in far:
        row = want_clamp[i][0, :, 1]
        assert len(np.unique(row)) > w // 2 and want_clamp[i].min() > 0, names[i]
    return far


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("mode", MODES)
def test_hostile_maps_on_every_window(gpu_vs, oracle, mode, fmt, shape):
    """part 1: the finite maps of HM.HOSTILE and HM.FILL_EXTREME and the far shifts as one batch per window and border; on the one-row frame
    also frame by frame through vs_bgr_image_warp"""
    vs, O = gpu_vs, oracle
    w, h = shape
    names, maps, src, want = _case(O, fmt, shape, mode)
    maxv = FORMATS[fmt][1]
    ts = [vs.Transform.of(*t) for t in maps]
    for border in BORDERS:
        for roi in WC.WINDOWS(w, h):
            x, y, rw, rh = roi
            got = vs.bgr_image_warp_roi_batch(src, ts, roi, mode=WC.MODES[mode], border=border, max_value=maxv)
            bad = _bad(names, got, want[border][:, y:y + rh, x:x + rw])
            assert not bad, (border, roi, bad)
        if h == 1:
            got = [vs.bgr_image_warp(src[i], ts[i], mode=WC.MODES[mode], border=border, max_value=maxv) for i in range(len(names))]
            assert not _bad(names, got, want[border]), border


@pytest.mark.parametrize("shape", SHAPES[:2], ids=["%dx%d" % s for s in SHAPES[:2]])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
@pytest.mark.parametrize("mode", MODES)
def test_far_rows(gpu_vs, oracle, mode, fmt, shape):
    """part 2: rows beyond each pitch's exactness limit in +y and -y, columns inside the frame, under the clamp: every tile's footprint fits
    the staged window and (restated decision, asserted) the guard refuses it.  The batch goes through the mode's usual route -- tables for the
    separable and contracted forms, the extents in the kernel for the others; the extents-only and the four-corner route of the same maps:
    test_calls_without_extents and test_calls_whose_tables_exceed_half_the_ring below.  Frame by frame as well: one-frame launches"""
    vs, O = gpu_vs, oracle
    w, h = shape
    names, maps, src, want = _case(O, fmt, shape, mode)
    maxv = FORMATS[fmt][1]
    far = _far_row_premise(names, want[O.BORDER_CLAMP], w)
    fmaps = [maps[i] for i in far]
    bits = 8 if fmt == "bgr8" else 16
    k = WC.launched_shape(WC.MODES[mode], bits, fmaps, w, h, (0, 0, w, h))
    n_guard = 0
    for t in fmaps:                                                  # the window would fit but for the guard, beyond this shape's pitch limit
        d = WC.decisions(t, w, h, (0, 0, w, h), k, True)[2]
        beyond = abs(t[3]) > WC.ROW_LIMIT[WC.SHAPES[k][4]] + 100
        assert (d[:, 5] <= WC.SHAPES[k][2]).all() and (d[:, 6] <= WC.SHAPES[k][3]).all() and d[:, 5].all()
        assert (not d[:, 2].any()) if beyond else True, (t, d)
        n_guard += beyond
    assert n_guard >= 6
    ts = [vs.Transform.of(*t) for t in fmaps]
    got = vs.bgr_image_warp_roi_batch(src[far], ts, (0, 0, w, h), mode=WC.MODES[mode], border=O.BORDER_CLAMP, max_value=maxv)
    bad = _bad([names[i] for i in far], got, want[O.BORDER_CLAMP][far])
    assert not bad, bad
    got = [vs.bgr_image_warp(src[i], vs.Transform.of(*maps[i]), mode=WC.MODES[mode], border=O.BORDER_CLAMP, max_value=maxv) for i in far]
    bad = _bad([names[i] for i in far], got, want[O.BORDER_CLAMP][far])
    assert not bad, ("frame by frame", bad)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("mode", MODES)
def test_maps_around_the_staged_windows_limits_and_the_launcher_s_thresholds(gpu_vs, oracle, mode, fmt):
    """part 3: the fit sweep -- zooms, turns and sub-pixel shifts that put tiles at each instantiation's staged rows and column groups and one
    beyond, maps on both sides of the 15.999-row and 64.99-column thresholds (premises: WC.sweep_premises, with the restated decision) -- as one
    batch (the standard window for all), then the threshold maps alone and in batches that mix sides"""
    vs, O = gpu_vs, oracle
    WC.sweep_premises()
    w, h = WC.SWEEP_SHAPE
    sweep = WC.fit_sweep()
    names = [n for n, _ in sweep]
    maxv = FORMATS[fmt][1]
    bits = 8 if fmt == "bgr8" else 16
    src = _content(fmt, len(sweep), w, h, seed=1)
    ts = [vs.Transform.of(*t) for _, t in sweep]
    by_name = {n: i for i, n in enumerate(names)}
    for border in BORDERS:
        want = _twin(O, src, [t for _, t in sweep], mode, border, maxv)
        for roi in WC.SWEEP_WINDOWS:
            x, y, rw, rh = roi
            got = vs.bgr_image_warp_roi_batch(src, ts, roi, mode=WC.MODES[mode], border=border, max_value=maxv)
            bad = _bad(names, got, want[:, y:y + rh, x:x + rw])
            assert not bad, (border, roi, bad[:8], len(bad))
        shapes = set()
        for bn, (members, _) in list(WC.MIXED_BATCHES.items()) + [(n, ([n], None)) for n, _ in WC.THRESHOLD_MAPS]:
            idx = [by_name[n] for n in members]
            shapes.add(WC.launched_shape(WC.MODES[mode], bits, [sweep[i][1] for i in idx], w, h, (0, 0, w, h)))
            got = vs.bgr_image_warp_roi_batch(src[idx], [ts[i] for i in idx], (0, 0, w, h), mode=WC.MODES[mode], border=border, max_value=maxv)
            bad = _bad(members, got, want[idx])
            assert not bad, (border, bn, bad)
        assert shapes == {"sep": {0, 1, 2}, "fast": {0, 1}, "lanczos2": {0}, "bilinear": {3 if bits == 8 else 4}}[mode], shapes


def _cycled_call(vs, O, mode, fmt, n, w, h, roi, border):
    """one call of n frames, frame i with map i of part 1's (the far rows first): every frame against the twin -> the names that differ"""
    maps = WC.hostile_maps(w, h)
    names = sorted(maps, key=lambda k: (k not in WC.far_rows(), k))
    maxv = FORMATS[fmt][1]
    dtype = FORMATS[fmt][0]
    rng = np.random.default_rng(n + w + maxv)
    src = rng.integers(maxv // 8, maxv - maxv // 8 + 1, (n, h, w, 3)).astype(dtype)
    assert src.min() > 0 and len({f.tobytes() for f in src}) == n
    per = [maps[names[i % len(names)]] for i in range(n)]
    want = _twin(O, src, per, mode, border, maxv)
    if border == O.BORDER_CLAMP:
        assert all((f > 0).mean() > 0.99 for f in want)
        for i in range(len(WC.far_rows())):
            assert want[i].min() > 0 and (len(np.unique(want[i][0, :, 1])) > w // 2 or w < 8), names[i]
    x, y, rw, rh = roi
    got = vs.bgr_image_warp_roi_batch(src, [vs.Transform.of(*t) for t in per], roi, mode=WC.MODES[mode], border=border, max_value=maxv)
    return [(i, names[i % len(names)]) for i in range(n) if not np.array_equal(got[i], want[i, y:y + rh, x:x + rw])]


@pytest.mark.parametrize("mode,fmt,border", [("sep", "bgr8", 0), ("sep", "bgr10", 1), ("fast", "bgr8", 0), ("lanczos2", "bgr8", 0), ("bilinear", "bgr8", 0),
                                             ("bilinear", "bgr10", 0)])
def test_calls_without_extents(gpu_vs, oracle, mode, fmt, border):
    """part 4, the four-corner route: 8193 frames of 66 x 3 -- one more than the parameter ring's half holds parameters and extents for
    (vs_capi_warp.hip: with_extents) -- so every tile's geometry comes from its four corners and no table is made; frame i has map i of part
    1's, the far rows first"""
    vs, O = gpu_vs, oracle
    n = WC.MAX_EXTENT_FRAMES + 1
    assert n == 8193 and 2 * n > WC.K_PARAM_SLOTS // 2 >= 2 * (n - 1)
    bad = _cycled_call(vs, O, mode, fmt, n, 66, 3, (0, 0, 66, 3), border)
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("mode,fmt,border", [("sep", "bgr8", 0), ("sep", "bgr10", 1), ("fast", "bgr8", 0)])
def test_calls_whose_tables_exceed_half_the_ring(gpu_vs, oracle, mode, fmt, border):
    """part 4, the extents-only route of the tabled forms: the most frames that still travel with extents, 8192, and the lowest one-column
    window whose tables (vs_warp_table.hpp: 16 bytes per 64 x 16 tile, 8 per row of the run padded to 4-row blocks) then exceed half the table
    ring (vs_call_plan.hpp: aligned_tables_fit) -- derived here: 225 rows.  The kernel keeps the extents and works the geometry out itself"""
    vs, O = gpu_vs, oracle
    n = WC.MAX_EXTENT_FRAMES
    rh = next(r for r in range(1, 4096) if not WC.tables_fit(n, 1, r))
    assert rh == 225 and WC.tables_fit(n, 1, rh - 1) and WC.table_ints(1, rh) == (16 * 15 + 8 * 228) // 4 == 516
    assert WC.tables_fit(8128, 1, rh) and not WC.tables_fit(8129, 1, rh)       # (at that window 8128 frames are the most that get tables)
    bad = _cycled_call(vs, O, mode, fmt, n, 5, rh, (2, 0, 1, rh), border)
    assert not bad, (len(bad), bad[:8])


def _dev_warp(vs, src, ts, roi, mode, border, maxv):
    """vs_bgr_image_warp_roi_batch on device memory: the source one element into its buffer at a pitch of 3 w + 7 (never on a dword: the rim
    fill), the destination window 3 elements into rows of 3 rw + 8 (never on a dword either), G guard rows above and below every frame and
    guard elements left and right of every row -> (n, rh, rw, 3); every guard element is looked at"""
    import torch
    n, h, w, c = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    x, y, rw, rh = roi
    ss, ds, left = c * w + 7, c * rw + 8, 3
    host = np.zeros(n * h * ss + 8, dtype)
    host[1:1 + n * h * ss].reshape(n, h, ss)[:, :, :c * w] = src.reshape(n, h, c * w)
    dfs = (rh + 2 * G) * ds
    guard = 0x5A if esz == 1 else 0x5A5A
    dhost = np.full(n * dfs + 8, guard, dtype)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda())
    dsrc, ddst = as_t(host), as_t(dhost)
    torch.cuda.synchronize()
    arr = (vs.Transform * n)(*ts)
    vs._check(vs.lib().vs_bgr_image_warp_roi_batch(C.c_void_p(dsrc.data_ptr() + esz), h * ss, n, w, h, ss, c, 8 * esz, arr, mode, border, maxv,
                                                   x, y, rw, rh, C.c_void_p(ddst.data_ptr() + (G * ds + left) * esz), dfs, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    assert (back[n * dfs:] == guard).all()
    frames = back[:n * dfs].reshape(n, rh + 2 * G, ds)
    res = frames[:, G:G + rh, left:left + c * rw].reshape(n, rh, rw, c).copy()
    frames[:, G:G + rh, left:left + c * rw] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination window were written"
    assert (frames[:, G + rh:] == guard).all(), "rows below a destination window were written"
    assert (frames[:, G:G + rh, :left] == guard).all(), "elements left of a destination row were written"
    assert (frames[:, G:G + rh, left + c * rw:] == guard).all(), "the tail of a destination row was written"
    return res


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("mode", MODES)
def test_unaligned_pitched_device_memory_inside_guard_bands(gpu_vs, oracle, mode, fmt, shape):
    """part 5: part 1's maps on its one-row windows, an inner window and the whole frame; device memory, neither buffer on a dword, both pitched"""
    vs, O = gpu_vs, oracle
    w, h = shape
    names, maps, src, want = _case(O, fmt, shape, mode)
    maxv = FORMATS[fmt][1]
    ts = [vs.Transform.of(*t) for t in maps]
    windows = [r for r in WC.WINDOWS(w, h) if r[3] == 1 or r[:2] == (5, 7)] + [(0, 0, w, h)]
    assert len(windows) >= 3
    for border in BORDERS:
        for roi in windows:
            x, y, rw, rh = roi
            got = _dev_warp(vs, src, ts, roi, WC.MODES[mode], border, maxv)
            bad = _bad(names, got, want[border][:, y:y + rh, x:x + rw])
            assert not bad, (border, roi, bad)
