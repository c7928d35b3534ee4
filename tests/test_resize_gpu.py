"""The resize pass on the GPU (include/vs_amd.h: vs_bgr_resize_batch; vs_resize.hip), bit for bit against the rule's restatement
(tests/_resize_ref.py): the smallest frames, sources and destinations around the kernel's tile (64 columns by up to 16 rows), every ratio the
rule names, mixed directions, both filters, 8-, 10-, 12- and 16-bit frames, pitched rows with guard words on both sides, host and device
memory, 0, 1 and 3 frames, and more frames than one grid holds."""

import numpy as np
import pytest

import _resize_ref as R

pytestmark = pytest.mark.gpu

G = 2                                                       # guard rows above and below every frame of a device buffer
FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}
FILTERS = {"linear": R.LINEAR, "area": R.AREA}


def frames(n, w, h, maxv, dtype, seed):
    """random frames with the extremes present"""
    a = np.random.default_rng(seed).integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)
    if a.size:
        a.reshape(-1)[0], a.reshape(-1)[-1] = maxv, 0
    return a


def banded(a, row_elems, stride, guard, lead):
    """frames (n, rows, row_elems) -> a flat buffer: `lead` elements in front, every frame G guard rows above and below, rows of `stride`"""
    n, rows, _ = a.shape
    buf = np.full(lead + n * (rows + 2 * G) * stride + 8, guard, a.dtype)
    buf[lead:lead + n * (rows + 2 * G) * stride].reshape(n, rows + 2 * G, stride)[:, G:G + rows, :row_elems] = a
    return buf


def dev_resize(vs, src, dw, dh, fmt, filt, src_guard, pad=(7, 5), lead=1):
    """vs_bgr_resize_batch on device memory, both buffers inside guard bands and pitched -> (n, dh, dw, 3).  The source's guard holds
    src_guard: a tap that strays shows in the result; the destination's guard must come back untouched"""
    import torch
    src = np.ascontiguousarray(src)
    n, sh, sw, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    ss, ds = 3 * sw + pad[0], 3 * dw + pad[1]
    guard = 0x5A if esz == 1 else 0x5A5A
    hsrc = banded(src.reshape(n, sh, 3 * sw), 3 * sw, ss, src_guard, lead)
    hdst = banded(np.full((n, dh, 3 * dw), guard, dtype), 3 * dw, ds, guard, lead)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda())
    dsrc, ddst = as_t(hsrc), as_t(hdst)
    torch.cuda.synchronize()
    vs.resize_batch_device(dsrc.data_ptr() + (lead + G * ss) * esz, (sh + 2 * G) * ss, n, sw, sh, ss, fmt, filt,
                           ddst.data_ptr() + (lead + G * ds) * esz, (dh + 2 * G) * ds, dw, dh, ds)
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    assert np.array_equal(dsrc.cpu().numpy().view(dtype), hsrc)                                     # the source is only read
    fr = back[lead:lead + n * (dh + 2 * G) * ds].reshape(n, dh + 2 * G, ds)
    res = fr[:, G:G + dh, :3 * dw].reshape(n, dh, dw, 3).copy()
    fr[:, G:G + dh, :3 * dw] = guard
    assert (back == guard).all(), "the destination was written outside its frames' rows"
    return res


def check(vs, sw, sh, dw, dh, filt, fmt="bgr8", n=1, seed=0, aligned=False):
    """aligned: the buffers start four elements into their allocations and the rows are dwords apart where dw is a multiple of 4; else one
    element in, odd pitches"""
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    src = frames(n, sw, sh, maxv, dtype, seed + sw * 7 + dh)
    want = R.resize(src, dw, dh, filt, maxv)
    got = dev_resize(vs, src, dw, dh, code, filt, src_guard=maxv // 2 + 1, **(dict(pad=(8, 4), lead=4) if aligned else {}))
    assert np.array_equal(got, want), (sw, sh, dw, dh, filt, fmt, int((got != want).sum()))
    return src, want


# ---- the smallest frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS.values(), ids=FILTERS.keys())
def test_the_smallest_frames(gpu_vs, filt):
    check(gpu_vs, 1, 1, 1, 1, filt)
    check(gpu_vs, 7, 5, 3, 2, filt)
    check(gpu_vs, 2, 2, 1, 1, filt)
    if filt == R.LINEAR:
        check(gpu_vs, 1, 1, 5, 3, filt)
        # rows of two, three and four pixels: below and at the eight elements that the two-taps-in-one-load form reads, pulled back from the end
        check(gpu_vs, 2, 3, 7, 5, filt)
        check(gpu_vs, 3, 3, 7, 5, filt)
        check(gpu_vs, 3, 2, 2, 2, filt)
        check(gpu_vs, 4, 4, 8, 8, filt)
        check(gpu_vs, 4, 3, 3, 3, filt, "bgr16")
    else:
        check(gpu_vs, 3, 3, 3, 3, filt)
        check(gpu_vs, 6, 4, 3, 2, filt, "bgr12")


# ---- around the tile: 64 columns, 16 rows (8, 4, 2, 1 where sixteen rows' source rows do not fit the LDS budget) -----------------------
@pytest.mark.parametrize("filt", FILTERS.values(), ids=FILTERS.keys())
def test_sources_and_destinations_around_the_tile(gpu_vs, filt):
    for dw in (63, 64, 65):
        for dh in (15, 16, 17):
            check(gpu_vs, 2 * dw - 1, 2 * dh - 1, dw, dh, filt, n=2)
    for sw in (63, 64, 65):
        for sh in (15, 16, 17):
            check(gpu_vs, sw, sh, 33, 9, filt, n=2)
    check(gpu_vs, 129, 33, 128, 32, filt)                   # two tiles each way, the second one full
    check(gpu_vs, 130, 35, 129, 33, filt)                   # ... and with one column and one row in a third
    # buffers whose rows start on dwords, as a caller's dense frames do; full tiles with and without a partial tile behind them
    for fmt in ("bgr8", "bgr10"):
        for dw in (60, 64, 68, 128, 132, 192):
            check(gpu_vs, 2 * dw - 1, 37, dw, 19, filt, fmt, n=2, aligned=True)           # shrinking: the direct form
            if filt == R.LINEAR:
                check(gpu_vs, dw - 9, 20, dw, 41, filt, fmt, n=2, aligned=True)           # growing: the tiled form


def tile_rows(s, dn, filt):
    """csrc/vs_resize.hpp's resize_tile_rows, restated: the largest of 16, 8, 4, 2, 1 rows whose source rows fit 64 rows of LDS"""
    for rows in (16, 8, 4, 2):
        if (((rows * s + dn - 2) // dn + 1) if filt == R.AREA else ((rows - 1) * s // dn + 3)) <= 64:
            return rows
    return 1


def test_tiles_lower_than_sixteen_rows(gpu_vs):
    """ratios at which sixteen destination rows touch more source rows than the LDS budget holds.  Premise: the launches of this test take
    tiles of 16, 8, 4, 2 and 1 rows"""
    dh, seen = 19, set()
    for ratio in (3, 5, 8, 20, 40, 70):
        for filt in (R.LINEAR, R.AREA):
            if R.axis_valid(dh * ratio, dh, filt):
                seen.add(tile_rows(dh * ratio, dh, filt))
                check(gpu_vs, 40, dh * ratio, 23, dh, filt, n=2)
    assert seen == {16, 8, 4, 2, 1}


# ---- the ratios the rule names ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_the_ratios(gpu_vs, fmt):
    vs = gpu_vs
    for filt in (R.LINEAR, R.AREA):
        check(vs, 8 * 9, 8 * 5, 9, 5, filt, fmt)            # 8:1 exactly
        check(vs, 37, 21, 37, 21, filt, fmt)                # 1:1
        check(vs, 74, 42, 37, 21, filt, fmt)                # 2:1
        check(vs, 96, 63, 64, 42, filt, fmt)                # 3:2
        check(vs, 70, 20, 9, 20, filt, fmt)                 # down on x only
        check(vs, 20, 70, 20, 9, filt, fmt)                 # down on y only
    check(vs, 100, 57, 107, 61, R.LINEAR, fmt)              # up by 1.07
    check(vs, 23, 11, 92, 44, R.LINEAR, fmt)                # up by 4
    check(vs, 64, 30, 21, 97, R.LINEAR, fmt)                # down on x, up on y
    check(vs, 21, 97, 64, 30, R.LINEAR, fmt)                # up on x, down on y
    check(vs, 200, 9, 3, 9, R.LINEAR, fmt)                  # LINEAR far beyond 8:1: two taps, the rest skipped


def test_one_source_pixel_past_eight_to_one_is_unsupported(gpu_vs):
    vs = gpu_vs
    src = np.zeros((1, 41, 73, 3), np.uint8)
    with pytest.raises(vs.VsError, match="error -3.*x axis"):
        vs.resize_batch(src[:, :40], 9, 5, vs.RESIZE_AREA)
    with pytest.raises(vs.VsError, match="error -3.*y axis"):
        vs.resize_batch(src[:, :, :72], 9, 5, vs.RESIZE_AREA)
    assert vs.resize_batch(src[:, :40, :72], 9, 5, vs.RESIZE_AREA).shape == (1, 5, 9, 3)


# ---- depths, memory, pitches, frame counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS.keys())
@pytest.mark.parametrize("filt", FILTERS.values(), ids=FILTERS.keys())
def test_every_depth_in_host_and_device_memory(gpu_vs, fmt, filt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    for n in (1, 3):
        src, want = check(vs, 83, 47, 31, 19, filt, fmt, n=n, seed=n)
        assert np.array_equal(vs.resize_batch(src, 31, 19, filt, fmt=code), want)
        guard = 0x5A if dtype == np.uint8 else 0x5A5A
        got, buf = vs.resize_batch(src, 31, 19, filt, fmt=code, src_stride=3 * 83 + 5, dst_stride=3 * 31 + 3, guard=guard)
        assert np.array_equal(got, want) and (buf[:, :, 3 * 31:] == guard).all()
    if filt == R.LINEAR:
        src, want = check(vs, 31, 19, 83, 47, filt, fmt, n=2)
        assert np.array_equal(vs.resize_batch(src, 83, 47, filt, fmt=code), want)


def test_no_frames_is_ok_and_launches_nothing(gpu_vs):
    vs = gpu_vs
    dst = np.full((1, 4, 15), 0x5A, np.uint8)
    r = vs.lib().vs_bgr_resize_batch(vs._p(np.zeros((1, 6, 24), np.uint8)), 6 * 24, 0, 8, 6, 24, vs.FMT_BGR8, vs.RESIZE_LINEAR, vs._p(dst), 60, 5, 4, 15, vs.MEM_HOST, None)
    assert r == 0 and (dst == 0x5A).all()


def test_the_same_size_is_the_identity_for_samples_up_to_the_maximum(gpu_vs):
    for fmt in ("bgr8", "bgr12", "bgr16"):
        for filt in (R.LINEAR, R.AREA):
            src, want = check(gpu_vs, 67, 18, 67, 18, filt, fmt, n=2)
            assert np.array_equal(want, src)


def test_more_frames_than_a_grid_holds(gpu_vs):
    """65 537 frames of 2 x 2 -> 1 x 1: the launch is cut at 65 535 frames; the frames behind the cut are resized like the ones in front"""
    import torch
    vs = gpu_vs
    n = 65537
    src = np.random.default_rng(11).integers(0, 256, (n, 2, 2, 3)).astype(np.uint8)
    want = ((src.astype(np.int64).sum(axis=(1, 2)) + 2) >> 2).astype(np.uint8)                       # consequence (d), factor 2
    assert np.array_equal(R.resize(src[-3:], 1, 1, R.AREA, 255).reshape(3, 3), want[-3:])
    dsrc = torch.from_numpy(src).cuda()
    for filt in (R.AREA, R.LINEAR):
        ddst = torch.full((n, 3), 0x5A, dtype=torch.uint8, device="cuda")
        vs.resize_batch_device(dsrc.data_ptr(), 12, n, 2, 2, 6, vs.FMT_BGR8, filt, ddst.data_ptr(), 3, 1, 1, 3)
        torch.cuda.synchronize()
        assert np.array_equal(ddst.cpu().numpy(), want), filt


def test_consecutive_calls_share_nothing(gpu_vs):
    """calls of different shapes back to back on one stream, read only at the end: every call's tables are its own span of the table ring"""
    import torch
    vs = gpu_vs
    shapes = [(50, 30, 20, 10, R.AREA), (20, 10, 50, 30, R.LINEAR), (64, 64, 8, 8, R.AREA), (9, 9, 9, 9, R.LINEAR), (33, 21, 30, 20, R.LINEAR)] * 3
    work = []
    for i, (sw, sh, dw, dh, filt) in enumerate(shapes):
        src = frames(2, sw, sh, 255, np.uint8, i)
        dsrc, ddst = torch.from_numpy(src).cuda(), torch.zeros((2, dh, dw, 3), dtype=torch.uint8, device="cuda")
        work.append((src, dsrc, ddst, dw, dh, filt))
    torch.cuda.synchronize()
    for src, dsrc, ddst, dw, dh, filt in work:
        _, sh, sw, _ = src.shape
        vs.resize_batch_device(dsrc.data_ptr(), sh * sw * 3, 2, sw, sh, 3 * sw, vs.FMT_BGR8, filt, ddst.data_ptr(), dh * dw * 3, dw, dh, 3 * dw)
    torch.cuda.synchronize()
    for src, dsrc, ddst, dw, dh, filt in work:
        assert np.array_equal(ddst.cpu().numpy(), R.resize(src, dw, dh, filt, 255))
