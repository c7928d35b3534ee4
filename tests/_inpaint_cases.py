"""Inputs and device-memory drivers for the inpaint's hostile tests (tests/test_inpaint_hostile_gpu.py, tests/test_cover_cpp.py; the premises
alone: tests/test_inpaint_cpu.py).  The discipline of tests/_hostile_maps.py: every builder ASSERTS ITS PREMISE on the CPU references alone
(tests/_fill_ref.py, tests/_inpaint_ref.py) -- the property that makes the input reach the code in question -- before anything is handed to a
kernel; where a premise fails, the input has to change, not the assertion.

Transforms are (A, B, TX, TY) tuples, as in tests/_hostile_maps.py."""
import numpy as np

import _fill_ref as RF
import _hostile_maps as HM
import _inpaint_ref as R

IDENT = (0.0, 0.0, 0.0, 0.0)
FAR = (0.0, 0.0, 5000.0, -3000.0)
ZOOM_IN = (0.25, 0.03, 2.0, -1.5)                                    # (the fill's test: every pixel of 300 x 270 has its four taps inside)
LIM = 1 << 29


def T(mod, rows):
    return [[mod.Transform.of(*t) for t in row] for row in rows]


def reference_index(O, cf, maps, w, h, roi=None):
    with np.errstate(all="ignore"):
        return R.coverage_batch(O, cf, T(O, maps), w, h, roi)


# ---- the rule on a window of a frame too large to enumerate ------------------------------------------------------------------------------------
def covered_window(O, t, w, h, roi):
    """-> ((rh, rw) bool: RF.covered(O, t, w, h) cropped to the window, computed on the window's rows and columns alone; small: every row
    origin (X0 + 16, Y0 + 16, wrapped) of the window's rows and every delta of its columns is below 2^29 in magnitude)"""
    x, y, rw, rh = roi
    X0, Y0, ad, bd = RF._table_terms(O, t, w, h, RF.cv_round_sat)
    X0, Y0, ad, bd = RF.wrap32(X0[y:y + rh] + 16), RF.wrap32(Y0[y:y + rh] + 16), ad[:, x:x + rw], bd[:, x:x + rw]
    sx, sy = RF.wrap32(X0 + ad) >> 10, RF.wrap32(Y0 + bd) >> 10
    small = all(int(np.abs(v).max()) < LIM for v in (X0, Y0, ad, bd))
    return RF._inside(sx, sy, w, h), small


# ---- the coverage index on device memory inside a guard band -----------------------------------------------------------------------------------
G = 3                                                                # guard rows in front of and behind every frame's index


def dev_coverage(vs, w, h, cf, maps, roi=None, aligned=True):
    """vs_bgr_fill_coverage_batch on device memory, every frame's index inside a guard band on four sides (G rows in front and behind, columns
    left and right) -> (n_out, rh, rw).  aligned: base, row stride and frame stride are multiples of 4 (the kernel's dword stores); else none
    of the rows starts on a dword.  The band must come back as it was"""
    import torch
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out = idx.shape[0]
    if aligned:
        gl, cs = 4, (rw + 8 + 3) & ~3
    else:
        gl, cs = 3, rw + 7 + (1 if (rw + 7) % 4 == 0 else 0)
    fs = (rh + 2 * G) * cs
    buf = torch.full((n_out * fs + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr() + G * cs + gl
    if not aligned:
        ptr += (5 - ptr % 4) % 4                                     # (the base one byte behind a dword; the buffer has eight bytes to spare)
    assert ((ptr | cs | fs) & 3 == 0) if aligned else (ptr & 3 == 1 and cs & 3 != 0)
    first = ptr - buf.data_ptr()                                     # the first index byte's place in the buffer
    torch.cuda.synchronize()
    vs.bgr_fill_coverage_batch_device(w, h, idx, T(vs, maps), (rx, ry, rw, rh), ptr, fs, cs)
    torch.cuda.synchronize()
    back = buf.cpu().numpy()
    shift = first - (G * cs + gl)                                    # 0 .. 3: the frames as laid out from there
    frames = back[shift:shift + n_out * fs].reshape(n_out, rh + 2 * G, cs)
    res = frames[:, G:G + rh, gl:gl + rw].copy()
    frames[:, G:G + rh, gl:gl + rw] = 0x5A
    assert (frames[:, :G] == 0x5A).all(), "rows in front of an index were written"
    assert (frames[:, G + rh:] == 0x5A).all(), "rows behind an index were written"
    assert (frames[:, G:G + rh, :gl] == 0x5A).all(), "columns left of an index were written"
    assert (frames[:, G:G + rh, gl + rw:] == 0x5A).all(), "columns right of an index were written"
    assert (back == 0x5A).all()
    return res


def check_index(vs, w, h, cf, maps, full, roi=None):
    """both pitch alignments against the crop of the full-frame reference; -> the frames that differ"""
    x, y, rw, rh = roi if roi is not None else (0, 0, w, h)
    want = full[:, y:y + rh, x:x + rw]
    bad = set()
    for aligned in (True, False):
        got = dev_coverage(vs, w, h, cf, maps, roi, aligned)
        assert got.shape == want.shape
        bad |= {o for o in range(len(want)) if not np.array_equal(got[o], want[o])}
    return sorted(bad)


# ---- coverage cases ------------------------------------------------------------------------------------------------------------------------------
def _strip_values(full):
    """the largest number of different index values in one 64 x 16 strip of the kernel's grid"""
    h, w = full.shape
    return max(len(np.unique(full[y0:y0 + 16, x0:x0 + 64])) for y0 in range(0, h, 16) for x0 in range(0, w, 64))


def _partly_covered_interior_strip(mask):
    """a 64 x 16 strip of the kernel's grid, inside a 256 x 256 block and off the frame's rim, that candidate 0 covers in part"""
    h, w = mask.shape
    for y0 in range(16, h - 32, 16):
        for x0 in range(64, w - 128, 64):
            if x0 % 256 == 0 or y0 % 256 == 0:
                continue
            if 0 < int(mask[y0:y0 + 16, x0:x0 + 64].sum()) < 16 * 64:
                return True
    return False


def rotation_case(O, w, h, n_cand):
    """four output frames whose candidates are all rotations up to +-0.5 rad with zooms 0.6 .. 1.6, one list cut by -1.  Premises: a
    block-interior 64 x 16 strip is partly covered by candidate 0; some strip holds at least three different index values; zeros occur"""
    rng = np.random.default_rng(7 * w + n_cand)
    n_out = 4
    maps = [[HM._rot(rng, w, h, big=True) for _ in range(n_cand)] for _ in range(n_out)]
    cf = rng.integers(0, 9, (n_out, n_cand)).astype(np.int32)
    cf[1, 2] = -1
    full = reference_index(O, cf, maps, w, h)
    assert any(_partly_covered_interior_strip(f == 1) for f in full)
    assert max(_strip_values(f) for f in full) >= 3
    assert (full == 0).any() and full[1].max() <= 2 and (full[[0, 2, 3]] > 2).any()
    return cf, maps, full


ROTATION_ROIS = [(13, 9, 1, 1), (37, 5, 63, 65), (5, 3, 65, 63), (41, 11, 256, 257), (43, 13, 257, 256), (7, 150, 257, 1), (150, 7, 1, 257), (199, 133, 65, 1)]


def rotation_rois(w, h):
    """windows with sides 1, 63, 65, 256 and 257 (cut to the frame) at offsets that are no multiples of 64"""
    rois = [(x, y, min(rw, w - x), min(rh, h - y)) for x, y, rw, rh in ROTATION_ROIS if x < w and y < h]
    assert all(x % 64 and y % 64 for x, y, _, _ in rois)
    if h > 257:
        assert {r[2] for r in rois} >= {1, 63, 65, 256, 257} and {r[3] for r in rois} >= {1, 63, 65, 256, 257}
    return rois


def hostile_case(O, w=64, h=48):
    """every map of HM.HOSTILE, HM.FILL_EXTREME and row0_trap once as candidate 0 in front of two ordinary candidates and once as candidate 1
    behind an ordinary candidate 0.  Premises: that candidate 0 covers between 30 % and 95 %; the near-singular maps are the ones on which
    int32 and int64 coverage part; the ordinary candidates behind row0_trap do cover something of row 0"""
    hostile = dict(HM.HOSTILE)
    hostile.update(HM.FILL_EXTREME)
    hostile["row0_trap"] = HM.row0_trap(O, w, h)
    names = sorted(hostile)
    with np.errstate(all="ignore"):
        for n in HM.NEAR_SINGULAR:
            t = O.Transform.of(*hostile[n])
            assert not np.array_equal(RF.covered(O, t, w, h), RF.covered_int64(O, t, w, h)), n
        own = (0.02, -0.03, 7.0, -5.0)
        assert 0.3 < RF.covered(O, O.Transform.of(*own), w, h).mean() < 0.95
    maps = [[hostile[n], (0.01, 0.02, -3.0, 2.0), IDENT] for n in names] + [[own, hostile[n], (0.0, 0.0, 0.25, -0.25)] for n in names]
    cf = np.array([[i % 4, (i + 1) % 4, (i + 2) % 4] for i in range(len(maps))], np.int32)
    full = reference_index(O, cf, maps, w, h)
    i = names.index("row0_trap")
    assert not (full[i, 0] == 1).any() and (full[i, 0] > 1).any()
    assert len(np.unique(full)) == 4
    label = [(names[k % len(names)], "as candidate %d" % (k // len(names))) for k in range(len(maps))]
    return cf, maps, full, label


def nothing_covered_cases(O):
    """1 x 9 and 9 x 1: no pixel has four taps inside, whatever the transform.  2 x 2: only source position (0, 0) has (premises)"""
    out = []
    for w, h in ((1, 9), (9, 1), (2, 2)):
        maps = [[IDENT, (0.0, 0.0, 0.25, 0.25), (0.0, 0.0, -0.5, 0.0)], [(0.0, 0.0, -0.25, -0.5), IDENT, (0.1, 0.2, 0.0, 0.0)], [(0.3, 0.0, 0.0, 0.0), IDENT, IDENT]]
        for row in maps:
            for t in row:
                cov = RF.covered(O, O.Transform.of(*t), w, h)
                sx, sy = RF.cv_source_ints(O, O.Transform.of(*t), w, h)
                assert not cov.any() if min(w, h) == 1 else ((sx[cov] == 0).all() and (sy[cov] == 0).all())
        cf = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]], np.int32)
        full = reference_index(O, cf, maps, w, h)
        assert not full.any() if min(w, h) == 1 else (full != 0).any()
        out.append((w, h, cf, maps, full))
    return out


def sixteen_case(O, w=300, h=270):
    """-> two cases of sixteen candidates.  Rim: candidates 1 .. 14 are far away and 15 is the identity, behind a candidate 0 that leaves a
    rim (premise: the value 16 occurs, 2 .. 15 do not, and the identity's last row and column stay 0).  Everything: candidate 0 is the zoom
    of the fill's test (premise: all ones)"""
    c0 = (0.02, -0.03, 7.0, -5.0)
    cf = np.arange(16, dtype=np.int32)[None]
    rim = [[c0] + [(0.0, 0.0, 5000.0 + 100 * k, -3000.0) for k in range(14)] + [IDENT]]
    full = reference_index(O, cf, rim, w, h)
    assert set(np.unique(full)) == {0, 1, 16} and (full == 16).sum() > 1000
    every = [[ZOOM_IN] + [FAR] * 14 + [IDENT]]
    ones = reference_index(O, cf, every, w, h)
    assert (ones == 1).all()
    return (cf, rim, full), (cf, every, ones)


def seam_case(O, n_cand, extra, w=12, h=9):
    """n_out = 4096 / n_cand + extra output frames: the C ABI uploads the entries in groups of 4096 / n_cand frames.  Premise: the frames on
    both sides of the seam have more than one value in their index"""
    group = 4096 // n_cand
    n_out = group + extra
    rng = np.random.default_rng(n_cand)
    cf = rng.integers(0, 6, (n_out, n_cand)).astype(np.int32)
    maps = [[(rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1), rng.uniform(-2, 2), rng.uniform(-2, 2)) for _ in range(n_cand)] for _ in range(n_out)]
    full = reference_index(O, cf, maps, w, h)
    assert all(len(np.unique(full[o])) > 1 for o in range(group - 2, n_out))
    assert len({full[o].tobytes() for o in range(group - 2, n_out)}) == extra + 2          # (and they differ from one another)
    return group, cf, maps, full


# ---- the push-pull on device memory inside a guard band ----------------------------------------------------------------------------------------
FORMATS = {"u8": (np.uint8, 255), "bgr10": (np.uint16, 1023), "bgr12": (np.uint16, 4095), "bgr16": (np.uint16, 65535)}


def fmt_code(vs, name):
    return {"u8": vs.FMT_BGR8, "bgr10": vs.FMT_BGR10, "bgr12": vs.FMT_BGR12, "bgr16": vs.FMT_BGR16_FULL}[name]


def dev_inpaint(vs, imgs, masks, fmt, g=2):
    """vs_bgr_inpaint_batch on device memory: every window and every mask inside a guard band on four sides, the frame strides larger than a
    frame -> (n, h, w, 3).  The band and the masks must come back as they were"""
    import torch
    imgs = np.ascontiguousarray(imgs)
    n, h, w, _ = imgs.shape
    dtype = imgs.dtype
    gv = 0x5A if dtype == np.uint8 else 0x5A5A
    big = np.full((n, h + 2 * g, (w + 2 * g) * 3 + 1), gv, dtype)
    big[:, g:g + h, 3 * g:3 * (g + w)] = imgs.reshape(n, h, 3 * w)
    mbig = np.full((n, h + 2 * g, w + 2 * g + 3), 0x77, np.uint8)
    mbig[:, g:g + h, g:g + w] = masks
    dimg = torch.from_numpy(big.view(np.int16) if dtype != np.uint8 else big).cuda()
    dmask = torch.from_numpy(mbig).cuda()
    torch.cuda.synchronize()
    stride, mstride, esz = big.shape[2], mbig.shape[2], big.itemsize
    vs.bgr_inpaint_batch_device(dimg.data_ptr() + (g * stride + 3 * g) * esz, (h + 2 * g) * stride, n, w, h, stride, fmt_code(vs, fmt),
                                dmask.data_ptr() + g * mstride + g, (h + 2 * g) * mstride, mstride)
    torch.cuda.synchronize()
    res = dimg.cpu().numpy().view(dtype)
    out = res[:, g:g + h, 3 * g:3 * (g + w)].reshape(n, h, w, 3).copy()
    res[:, g:g + h, 3 * g:3 * (g + w)] = gv
    assert (res == gv).all(), "the guard band around a window was written"
    assert np.array_equal(dmask.cpu().numpy(), mbig), "a mask was written"
    return out


def check_inpaint(vs, imgs, masks, fmt, want=None, host=False):
    """the GPU's result against the rule (want: R.inpaint_batch(imgs, masks) where the caller has it already), and directly, independent of
    the reference: (a) kept pixels come back bit for bit; (b) per channel, every sample lies within the minimum and maximum of the frame's
    kept samples; (e) two different junk fills of the open pixels give the same bytes (a frame without a kept pixel comes back as it went
    in: junk and all).  -> the frames that differ from the rule"""
    dtype = imgs.dtype
    keep = np.asarray(masks) != 0
    if want is None:
        want = R.inpaint_batch(imgs, masks)
    rng = np.random.default_rng(imgs.shape[1] * 7 + imgs.shape[2])
    top = int(np.iinfo(dtype).max)
    junk = [np.where(keep[..., None], imgs, rng.integers(0, top + 1, imgs.shape).astype(dtype)).astype(dtype),
            np.where(keep[..., None], imgs, np.asarray(top - 3, dtype)).astype(dtype)]
    run = (lambda a: vs.bgr_inpaint_batch(a, masks, fmt=fmt_code(vs, fmt))) if host else (lambda a: dev_inpaint(vs, a, masks, fmt))
    got = [run(a) for a in junk]
    bad = set()
    for k in range(len(imgs)):
        if not keep[k].any():
            assert np.array_equal(got[0][k], junk[0][k]) and np.array_equal(got[1][k], junk[1][k]), ("a window without a kept pixel was written", k)
            continue
        assert np.array_equal(got[0][k][keep[k]], imgs[k][keep[k]]) and np.array_equal(got[1][k][keep[k]], imgs[k][keep[k]]), ("(a): a kept pixel changed", k)
        lo, hi = imgs[k][keep[k]].min(0), imgs[k][keep[k]].max(0)
        assert (got[0][k] >= lo).all() and (got[0][k] <= hi).all(), ("(b): a sample outside the kept samples' range", k)
        assert np.array_equal(got[0][k], got[1][k]), ("(e): the result depends on what the open pixels held", k)
        if not np.array_equal(got[0][k], want[k]):
            bad.add(k)
    return sorted(bad)


def corner_and_single_masks(w, h):
    """one kept pixel in each of the four corners and in the centre; one open pixel at (0, 0) and at (h - 1, w - 1), and in the last column
    of the middle row"""
    out = []
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1 + (x + y) % 255
        out.append(m)
    for y, x in ((0, 0), (h - 1, w - 1), (h // 2, w - 1)):
        m = np.full((h, w), 9, np.uint8)
        m[y, x] = 0
        out.append(m)
    return np.stack(out)


def two_level_content(rng, n, w, h, dtype, lo):
    """samples in {lo, lo + 1}: every mean and every interpolation lies between two neighbouring integers, and the rounding decides"""
    return (lo + rng.integers(0, 2, (n, h, w, 3))).astype(dtype)


def inpaint_variant(img, mask, floor_mean=False, pull_without_8=False):
    """tests/_inpaint_ref.py's inpaint with one of the rule's two roundings taken out: NOT the rule.  For the premise that an input tells the
    rule from them"""
    m = np.asarray(mask) != 0
    levels = [(np.asarray(img).astype(np.int64), m)]
    while levels[-1][1].shape != (1, 1):
        v, mm = levels[-1]
        H, W = mm.shape
        H1, W1 = (H + 1) >> 1, (W + 1) >> 1
        vp, mp = np.zeros((2 * H1, 2 * W1, 3), np.int64), np.zeros((2 * H1, 2 * W1), bool)
        vp[:H, :W], mp[:H, :W] = np.where(mm[..., None], v, 0), mm
        n = mp.reshape(H1, 2, W1, 2).sum((1, 3)).astype(np.int64)
        s = vp.reshape(H1, 2, W1, 2, 3).sum((1, 3))
        nn = np.maximum(n, 1)[..., None]
        levels.append((np.where(n[..., None] > 0, s // nn if floor_mean else (2 * s + nn) // (2 * nn), 0), n > 0))
    if not levels[-1][1][0, 0]:
        return np.array(img, copy=True)
    up = levels[-1][0]
    for v, mm in reversed(levels[:-1]):
        py, qy = R._near_far(mm.shape[0], up.shape[0])
        px, qx = R._near_far(mm.shape[1], up.shape[1])
        est = (9 * up[py][:, px] + 3 * up[py][:, qx] + 3 * up[qy][:, px] + up[qy][:, qx] + (0 if pull_without_8 else 8)) >> 4
        up = np.where(mm[..., None], v, est)
    return np.where(m[..., None], img, up.astype(img.dtype))


def rounding_case(w, h, fmt, high, open_share):
    """content in {0, 1} or {maxv - 1, maxv} under a random mask.  Premise: a floor mean in the push and a pull without its + 8 each give a
    different result on this input (and the unchanged variant IS the reference)"""
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(w + 3 * h + maxv + int(100 * open_share) + high)
    img = two_level_content(rng, 1, w, h, dtype, maxv - 1 if high else 0)
    mask = ((rng.random((1, h, w)) >= open_share) * rng.integers(1, 256, (1, h, w))).astype(np.uint8)
    want = R.inpaint_batch(img, mask)
    assert np.array_equal(inpaint_variant(img[0], mask[0]), want[0])
    assert not np.array_equal(inpaint_variant(img[0], mask[0], floor_mean=True), want[0])
    assert not np.array_equal(inpaint_variant(img[0], mask[0], pull_without_8=True), want[0])
    return img, mask, want


def out_of_range_case(w, h, fmt):
    """a 10- or 12-bit container that holds 65535 and max_value + 1 at scattered KEPT pixels, kept mask bytes 0x80 and 0xFF; the last frame's
    kept samples are all 65535.  Premises: samples above max_value occur among the inpainted ones, and that last frame comes back as 65535
    everywhere"""
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(maxv + w)
    n = 3
    img = rng.integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)
    keep = rng.random((n, h, w)) < 0.4
    keep[1] = rng.random((h, w)) < 0.03
    mask = np.where(keep, np.where(rng.random((n, h, w)) < 0.5, 0x80, 0xFF), 0).astype(np.uint8)
    img[rng.random((n, h, w)) < 0.08] = 65535
    img[rng.random((n, h, w, 3)) < 0.05] = maxv + 1
    img[2][keep[2]] = 65535
    assert all((img[k][keep[k]] == 65535).any() and (img[k][keep[k]] == maxv + 1).any() for k in range(2))
    assert set(np.unique(mask)) == {0, 0x80, 0xFF}
    want = R.inpaint_batch(img, mask)
    assert all((want[k][~keep[k]] > maxv).any() for k in range(n)) and (want[2] == 65535).all() and not (img[2] == 65535).all()
    return img, mask, want


def idle_and_busy_batch(w, h, fmt):
    """seven frames: [all kept, busy, all open, busy, one open, one kept, busy]; -> (imgs, masks, want)"""
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(w + maxv)
    imgs = rng.integers(0, maxv + 1, (7, h, w, 3)).astype(dtype)
    masks = ((rng.random((7, h, w)) < 0.5) * 255).astype(np.uint8)
    masks[0], masks[2], masks[4], masks[5] = 0x80, 0, 1, 0
    masks[4, h - 1, w - 1] = 0
    masks[5, h // 3, w - 1] = 200
    want = R.inpaint_batch(imgs, masks)
    opens = [int((m == 0).sum()) for m in masks]
    assert opens[0] == 0 and opens[2] == w * h and opens[4] == 1 and opens[5] == w * h - 1 and all(0 < opens[k] < w * h for k in (1, 3, 6))
    assert all(np.array_equal(want[k], imgs[k]) == (k in (0, 2)) for k in range(7))
    return imgs, masks, want


def inpaint_2x2(imgs, masks):
    """the rule on 2 x 2 windows, all frames at once: one push to 1 x 1, and a pull whose four taps are that one texel -- (16 P + 8) >> 4 = P:
    every open pixel becomes the rounded mean of the kept ones"""
    keep = masks != 0
    n = keep.sum((1, 2)).astype(np.int64)
    s = np.where(keep[..., None], imgs, 0).astype(np.int64).sum((1, 2))
    nn = np.maximum(n, 1)[:, None]
    mean = ((2 * s + nn) // (2 * nn)).astype(imgs.dtype)
    out = np.where(keep[..., None], imgs, mean[:, None, None, :])
    return np.where((n > 0)[:, None, None, None], out, imgs)
