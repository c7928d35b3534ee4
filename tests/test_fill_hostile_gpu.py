"""The border fill's pass 2 (vs_fill.hip) where the first tests never went: several 256 x 256 blocks, coverage boundaries that cross block
and strip seams diagonally, windows of 1 .. 257 pixels at odd offsets, frames in which nothing can be covered, NaN / singular / near-singular
/ saturating maps as candidate 0 and as later candidates, samples above max_value, the C ABI's group seam -- bit for bit against the rule's
reference (tests/_fill_ref.py: the oracle's plain warp plus the rule's int32 coverage).  Inputs and premises: tests/_hostile_maps.py.

The kernel-level calls work on DEVICE memory with the destination inside a guard band on all four sides (the host-memory form copies only
the rows' own bytes back)."""
import ctypes as C

import numpy as np
import pytest

import _fill_ref as RF
import _hostile_maps as HM

pytestmark = pytest.mark.gpu

G = 3
KINDS = [(8, 255, np.uint8), (10, 1023, np.uint16)]
IDENT = (0.0, 0.0, 0.0, 0.0)


def _dev_fill(vs, src, cf, maps, roi=None, border=None, maxv=None, ss=None, ds=None):
    """vs_bgr_image_warp_fill_batch on device memory, the destination windows G rows apart inside a guard-filled buffer -> (n_out, rh, rw, 3)"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    ss = 3 * w if ss is None else ss
    ds = 3 * rw if ds is None else ds
    host = np.zeros((n_src, h, ss), dtype)
    host[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out, n_cand = idx.shape
    flat = [vs.Transform.of(*t) for row in maps for t in row]
    assert len(flat) == n_out * n_cand
    arr = (vs.Transform * len(flat))(*flat)
    dfs = (rh + 2 * G) * ds
    guard = 0x5A if esz == 1 else 0x5A5A
    dhost = np.full(n_out * dfs + 8, guard, dtype)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda())
    dsrc, ddst = as_t(host), as_t(dhost)
    torch.cuda.synchronize()
    vs._check(vs.lib().vs_bgr_image_warp_fill_batch(C.c_void_p(dsrc.data_ptr()), h * ss, n_src, w, h, ss, 3, 8 * esz, n_out, n_cand,
                                                    idx.ctypes.data_as(C.POINTER(C.c_int32)), arr, vs.BORDER_CONSTANT if border is None else border,
                                                    maxv if maxv is not None else (255 if esz == 1 else 65535), rx, ry, rw, rh,
                                                    C.c_void_p(ddst.data_ptr() + G * ds * esz), dfs, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    frames = back[:n_out * dfs].reshape(n_out, rh + 2 * G, ds)
    res = frames[:, G:G + rh, :3 * rw].reshape(n_out, rh, rw, 3).copy()
    frames[:, G:G + rh, :3 * rw] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination window were written"
    assert (frames[:, G + rh:] == guard).all(), "rows below a destination window were written"
    assert (frames[:, G:G + rh, 3 * rw:] == guard).all(), "the tail of a destination row was written"
    assert (back == guard).all()
    return res


def _ref(O, src, cf, maps, border, maxv, roi=None):
    with np.errstate(all="ignore"):
        return RF.fill_batch(O, src, cf, [[O.Transform.of(*t) for t in row] for row in maps], border, maxv, roi)


def _frames(rng, n, w, h, dtype, maxv):
    base = rng.integers(0, maxv + 1, (n, h // 8 + 2, w // 8 + 2, 3))
    up = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :h, :w]
    return np.clip(up + rng.integers(-3, 4, up.shape), 0, maxv).astype(dtype)


def _big_rotations(rng, n_out, n_cand, w, h):
    """rotations up to +-0.5 rad with zooms 0.6 .. 1.6, for candidate 0 and for the others"""
    return [[HM._rot(rng, w, h, big=True) for _ in range(n_cand)] for _ in range(n_out)]


def _partly_covered_interior_strip(mask):
    """a 64 x 16 strip of the kernel's grid, inside a 256 x 256 block and off the frame's rim, that candidate 0 covers in part"""
    h, w = mask.shape
    for y0 in range(16, h - 32, 16):
        for x0 in range(64, w - 128, 64):
            if x0 % 256 == 0 or y0 % 256 == 0:
                continue
            n = int(mask[y0:y0 + 16, x0:x0 + 64].sum())
            if 0 < n < 16 * 64:
                return True
    return False


@pytest.mark.parametrize("shape", [(300, 270), (520, 70)], ids=["300x270", "520x70"])
@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10"])
def test_blocks_strips_and_windows_under_large_rotations(gpu_vs, oracle, bits, maxv, dtype, shape):
    """2 x 2 and 3 x 1 blocks; the covered region's boundary crosses block and strip seams diagonally (premise: a block-interior strip is
    covered in part); full frames under both borders with pitched rows, and windows whose sides are 1, 63, 65, 256 and 257 at offsets that
    are no multiples of 64: each equals the crop of the full result"""
    vs, O = gpu_vs, oracle
    w, h = shape
    rng = np.random.default_rng(w + bits)
    n_src, n_out, n_cand = 5, 4, 4
    src = _frames(rng, n_src, w, h, dtype, maxv)
    maps = _big_rotations(rng, n_out, n_cand, w, h)
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    cf[1, 2] = -1
    masks = [RF.covered(O, O.Transform.of(*row[0]), w, h) for row in maps]
    assert any(_partly_covered_interior_strip(m) for m in masks)
    assert sum(0 < m.mean() < 1 for m in masks) >= 2
    full = {}
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        full[border] = want = _ref(O, src, cf, maps, border, maxv)
        got = _dev_fill(vs, src, cf, maps, border=border, maxv=maxv)
        assert np.array_equal(got, want), (border, int((got != want).sum()))
        got = _dev_fill(vs, src, cf, maps, border=border, maxv=maxv, ss=3 * w + 7, ds=3 * w + 5)
        assert np.array_equal(got, want), (border, "pitched")
    plain = _ref(O, src, cf[:, :1], [r[:1] for r in maps], vs.BORDER_CONSTANT, maxv)
    assert (plain != full[vs.BORDER_CONSTANT]).mean() > 0.01       # the candidates fill something
    sides = (1, 63, 65, 256, 257)
    rois = [(13, 9, 1, 1), (37, 5, 63, 65), (5, 3, 65, 63), (41, 11, 256, 257), (43, 13, 257, 256), (7, 150, 257, 1), (150, 7, 1, 257), (199, 133, 65, 1)]
    rois = [(x, y, min(rw, w - x), min(rh, h - y)) for x, y, rw, rh in rois if x < w and y < h]
    assert all(x % 64 and y % 64 for x, y, _, _ in rois)
    if h > 257:
        assert {r[2] for r in rois} >= set(sides) and {r[3] for r in rois} >= set(sides)
    for i, (x, y, rw, rh) in enumerate(rois):
        border = (vs.BORDER_CONSTANT, vs.BORDER_CLAMP)[i % 2]
        got = _dev_fill(vs, src, cf, maps, roi=(x, y, rw, rh), border=border, maxv=maxv, ds=3 * rw + (i % 3))
        want = full[border][:, y:y + rh, x:x + rw]
        assert np.array_equal(got, want), ((x, y, rw, rh), int((got != want).sum()))


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10"])
def test_frames_in_which_nothing_or_one_position_can_be_covered(gpu_vs, oracle, bits, maxv, dtype):
    """1 x 9 and 9 x 1: no pixel has four taps inside, whatever the transform.  2 x 2: only source position (0, 0) has (premises)"""
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(bits)
    for w, h in ((1, 9), (9, 1), (2, 2)):
        src = rng.integers(0, maxv + 1, (3, h, w, 3)).astype(dtype)
        maps = [[IDENT, (0.0, 0.0, 0.25, 0.25), (0.0, 0.0, -0.5, 0.0)], [(0.0, 0.0, -0.25, -0.5), IDENT, (0.1, 0.2, 0.0, 0.0)], [(0.3, 0.0, 0.0, 0.0), IDENT, IDENT]]
        for row in maps:
            for t in row:
                cov = RF.covered(O, O.Transform.of(*t), w, h)
                sx, sy = RF.cv_source_ints(O, O.Transform.of(*t), w, h)
                assert not cov.any() if min(w, h) == 1 else ((sx[cov] == 0).all() and (sy[cov] == 0).all())
        cf = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]], np.int32)
        for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
            want = _ref(O, src, cf, maps, border, maxv)
            got = _dev_fill(vs, src, cf, maps, border=border, maxv=maxv)
            assert np.array_equal(got, want), (w, h, border)


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10"])
def test_candidate_0_covering_everything_is_the_plain_roi_warp(gpu_vs, oracle, bits, maxv, dtype):
    """a zoom into the frame: every pixel's four taps are inside (premise), so pass 2 leaves every block at its first test -- with sixteen
    candidates listed"""
    vs, O = gpu_vs, oracle
    w, h = 300, 270
    rng = np.random.default_rng(bits + 1)
    src = _frames(rng, 4, w, h, dtype, maxv)
    zoom = (0.25, 0.03, 2.0, -1.5)
    assert RF.covered(O, O.Transform.of(*zoom), w, h).all()
    cf = np.array([[1] + [int(v) for v in rng.integers(0, 4, 15)]], np.int32)
    maps = [[zoom] + [HM._rot(rng, w, h, big=True) for _ in range(15)]]
    for roi in ((0, 0, w, h), (21, 17, 257, 129)):
        plain = vs.bgr_image_warp_roi_batch(src[1][None], [vs.Transform.of(*zoom)], roi, mode=vs.WARP_BILINEAR_CV, border=vs.BORDER_CONSTANT, max_value=maxv)
        got = _dev_fill(vs, src, cf, maps, roi=roi, maxv=maxv)
        assert np.array_equal(got, plain)
        assert np.array_equal(got, _ref(O, src, cf, maps, vs.BORDER_CONSTANT, maxv, roi))


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10"])
def test_hostile_maps_as_candidate_0_and_as_later_candidates(gpu_vs, oracle, bits, maxv, dtype):
    """NaN, infinite, singular, near-singular, quarter-turn maps; translations beyond the 2^29 table-term guard, beyond cvRound's saturation
    and beyond everything; the near-singular transforms on which int64 and int32 coverage part (premise) -- each once as candidate 0 in
    front of two ordinary candidates and once as candidate 1 behind an ordinary candidate 0 that leaves a border"""
    vs, O = gpu_vs, oracle
    w, h = 64, 48
    rng = np.random.default_rng(3 * bits)
    src = _frames(rng, 4, w, h, dtype, maxv)
    hostile = dict(HM.HOSTILE)
    hostile.update(HM.FILL_EXTREME)
    hostile["row0_trap"] = HM.row0_trap(vs, w, h)
    for n in HM.NEAR_SINGULAR:
        t = O.Transform.of(*hostile[n])
        assert not np.array_equal(RF.covered(O, t, w, h), RF.covered_int64(O, t, w, h)), n
    names = sorted(hostile)
    own = (0.02, -0.03, 7.0, -5.0)
    assert 0.3 < RF.covered(O, O.Transform.of(*own), w, h).mean() < 0.95
    maps = [[hostile[n], (0.01, 0.02, -3.0, 2.0), IDENT] for n in names] + [[own, hostile[n], (0.0, 0.0, 0.25, -0.25)] for n in names]
    cf = np.array([[i % 4, (i + 1) % 4, (i + 2) % 4] for i in range(len(maps))], np.int32)
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        want = _ref(O, src, cf, maps, border, maxv)
        got = _dev_fill(vs, src, cf, maps, border=border, maxv=maxv)
        bad = [(names[i % len(names)], i // len(names)) for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (border, bad)
    # one-row windows at frame row 0: a rectangle there has equal row terms at both ends, and only the deltas can be extreme
    for roi in ((0, 0, w, 1), (3, 0, 33, 1), (0, 0, 1, h)):
        want = _ref(O, src, cf, maps, vs.BORDER_CONSTANT, maxv, roi)
        got = _dev_fill(vs, src, cf, maps, roi=roi, maxv=maxv)
        bad = [(names[i % len(names)], i // len(names)) for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (roi, bad)
    i = names.index("row0_trap")                                     # the premise of that case: the later candidates do fill row 0
    plain = _ref(O, src, cf[i:i + 1, :1], [maps[i][:1]], vs.BORDER_CONSTANT, maxv, (0, 0, w, 1))
    assert not np.array_equal(plain, _ref(O, src, cf[i:i + 1], [maps[i]], vs.BORDER_CONSTANT, maxv, (0, 0, w, 1)))


def test_samples_above_max_value_in_a_later_candidate(gpu_vs, oracle):
    """a bgr10 container that holds 65535 at scattered pixels, max_value 1023: the 16-bit sampler's saturation is live (premise: the fill
    under max_value 65535 differs from the fill under 1023)"""
    vs, O = gpu_vs, oracle
    w, h = 131, 77
    rng = np.random.default_rng(10)
    src = _frames(rng, 3, w, h, np.uint16, 1023)
    src[1][rng.random((h, w)) < 0.1] = 65535
    src[2][rng.random((h, w, 3)) < 0.1] = 1024
    maps = [[(0.03, -0.04, 11.0, -8.0), (0.0, 0.01, 0.3, 0.6), (0.01, 0.0, -0.4, 0.2)], [(-0.02, 0.05, -9.0, 6.0), (0.0, 0.0, 0.5, 0.5), IDENT]]
    cf = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    want = _ref(O, src, cf, maps, vs.BORDER_CONSTANT, 1023)
    loose = _ref(O, src, cf, maps, vs.BORDER_CONSTANT, 65535)
    assert (loose > 1023).any() and want.max() == 1023 and not np.array_equal(want, loose)
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        got = _dev_fill(vs, src, cf, maps, border=border, maxv=1023)
        assert np.array_equal(got, _ref(O, src, cf, maps, border, 1023))


K_SLOTS = 1 << 15                                                    # the parameter ring's slots (the group sizes)


@pytest.mark.parametrize("n_cand,extra", [(16, 3), (1, 1)])
def test_the_second_group_of_a_long_call(gpu_vs, oracle, n_cand, extra):
    """the warp / fill path uploads per-frame parameters in groups of min(kSlots / 2 / 3, (kSlots / 2 / 4) / n_cand) output frames: 256 at
    16 candidates, 4096 at 1.  n_out = group + extra crosses the seam: the second group's source and destination offsets and ring spans"""
    vs, O = gpu_vs, oracle
    group = min(K_SLOTS // 2 // 3, (K_SLOTS // 2 // 4) // n_cand)
    assert group == {16: 256, 1: 4096}[n_cand]
    n_out = group + extra
    assert n_out > group
    w, h, n_src = 12, 9, 6
    rng = np.random.default_rng(n_cand)
    src = _frames(rng, n_src, w, h, np.uint8, 255)
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    maps = [[(rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1), rng.uniform(-2, 2), rng.uniform(-2, 2)) for _ in range(n_cand)] for _ in range(n_out)]
    want = _ref(O, src, cf, maps, vs.BORDER_CONSTANT, 255)
    if n_cand > 1:                                                   # frames on both sides of the seam are filled from their candidates
        plain = _ref(O, src, cf[:, :1], [r[:1] for r in maps], vs.BORDER_CONSTANT, 255)
        assert all((plain[o] != want[o]).any() for o in range(group - 2, n_out))
    got = _dev_fill(vs, src, cf, maps, maxv=255)
    bad = [o for o in range(n_out) if not np.array_equal(got[o], want[o])]
    assert not bad, (bad[:8], len(bad))
