"""The inpaint's two kernel-level calls on the GPU (include/vs_amd.h: vs_bgr_fill_coverage_batch, vs_bgr_inpaint_batch) against the rule's
restatement (tests/_inpaint_ref.py; tests/test_inpaint_cpu.py holds it against a second one): bytes for bytes, np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import _inpaint_ref as R

pytestmark = pytest.mark.gpu


def _gt(vs, t):
    return vs.Transform.of(*t.tup())


def _cands(O, rng, n_out, n_cand, w, h):
    """candidate lists with shifts, rotation and zoom; lists cut short by -1; output 0's own frame covers everything but the frame's last
    row and column (the identity), output 1's nothing"""
    cf = rng.integers(0, 7, (n_out, n_cand)).astype(np.int32)
    ct = []
    for o in range(n_out):
        own = (rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-0.12, 0.12) * w, rng.uniform(-0.12, 0.12) * h)
        if o == 0:
            own = (0.0, 0.0, 0.0, 0.0)
        if o == 1:
            own = (0.0, 0.0, 5000.0, -3000.0)
        row = [O.Transform.of(*own)]
        for c in range(1, n_cand):
            row.append(O.Transform.of(own[0] + rng.uniform(-0.03, 0.03), own[1] + rng.uniform(-0.02, 0.02),
                                      own[2] % 50 + rng.uniform(-0.1, 0.1) * w, own[3] % 50 + rng.uniform(-0.1, 0.1) * h))
        ct.append(row)
        if n_cand >= 3 and o % 2 == 1:
            cf[o, rng.integers(1, n_cand)] = -1                     # the list ends early
    return cf, ct


ROIS = {(300, 270): [None, (13, 9, 257, 256), (37, 5, 63, 65), (7, 11, 65, 1), (3, 3, 1, 63), (21, 7, 256, 257), (1, 2, 298, 267)],
        (520, 70): [None, (131, 3, 257, 65), (70, 2, 256, 63), (11, 1, 65, 1), (259, 5, 1, 65), (1, 1, 63, 63), (3, 0, 513, 69)]}


@pytest.mark.parametrize("n_cand", [1, 2, 5, 16])
@pytest.mark.parametrize("w,h", sorted(ROIS))
def test_coverage_index_equals_the_rule(gpu_vs, oracle, w, h, n_cand):
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(100 * n_cand + w)
    n_out = 5
    cf, ct = _cands(O, rng, n_out, n_cand, w, h)
    gct = [[_gt(vs, t) for t in row] for row in ct]
    full = R.coverage_batch(O, cf, ct, w, h)
    assert (full[0, :-1, :-1] == 1).all() and not (full[1] == 1).any()
    if n_cand >= 5:
        assert len(np.unique(full)) >= 4                             # the test has teeth: several candidates, and pixels none covers
    for k, roi in enumerate(ROIS[(w, h)]):
        x, y, rw, rh = roi if roi is not None else (0, 0, w, h)
        want = full[:, y:y + rh, x:x + rw]
        got = vs.bgr_fill_coverage_batch(w, h, cf, gct, roi=roi)
        assert np.array_equal(got, want), (roi, int((got != want).sum()))
        # pitched rows, dword-aligned or not, inside a guard value
        got, raw = vs.bgr_fill_coverage_batch(w, h, cf, gct, roi=roi, cov_stride=rw + (4 - rw % 4 if k % 2 else 5), guard=0x5A)
        assert np.array_equal(got, want) and (raw[:, :, rw:] == 0x5A).all(), roi


def test_coverage_in_device_memory(gpu_vs, oracle):
    import torch
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(3)
    w, h, n_out, n_cand = 300, 270, 4, 5
    cf, ct = _cands(O, rng, n_out, n_cand, w, h)
    gct = [[_gt(vs, t) for t in row] for row in ct]
    roi = (13, 9, 257, 256)
    want = R.coverage_batch(O, cf, ct, w, h, roi)
    for stride, pad in ((260, 4), (259, 3)):
        buf = torch.full((n_out * 256 * stride + 2 * pad,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vs.bgr_fill_coverage_batch_device(w, h, cf, gct, roi, buf.data_ptr() + pad, 256 * stride, stride)
        torch.cuda.synchronize()
        res = buf.cpu().numpy()
        body = res[pad:pad + n_out * 256 * stride].reshape(n_out, 256, stride)
        assert np.array_equal(body[:, :, :257], want)
        assert (res[:pad] == 0x5A).all() and (res[pad + n_out * 256 * stride - (stride - 257):] == 0x5A).all() and (body[:, :-1, 257:] == 0x5A).all()


def test_coverage_argument_errors(gpu_vs):
    vs = gpu_vs
    t = vs.Transform.of(0, 0, 3, 2)
    assert vs.bgr_fill_coverage_batch(48, 32, [[0, 1]], [[t, t]]).shape == (1, 32, 48)
    for bad in (lambda: vs.bgr_fill_coverage_batch(48, 32, np.zeros((1, 0), np.int32), [[]]),           # n_cand 0
                lambda: vs.bgr_fill_coverage_batch(48, 32, [[0] * 17], [[t] * 17]),                      # n_cand 17
                lambda: vs.bgr_fill_coverage_batch(48, 32, [[-1, 1]], [[t, t]]),                         # candidate 0 is the frame itself
                lambda: vs.bgr_fill_coverage_batch(48, 32, [[0]], [[t]], roi=(40, 0, 9, 4)),             # a window outside the frame
                lambda: vs.bgr_fill_coverage_batch(48, 32, [[0]], [[t]], cov_stride=47)):
        with pytest.raises(vs.VsError, match=r"error -1.*vs_bgr_fill_coverage_batch"):
            bad()
    with pytest.raises(vs.VsError, match="error -3"):
        vs.bgr_fill_coverage_batch(40000, 32, [[0]], [[t]])
    with pytest.raises(vs.VsError, match=r"error -1.*vs_bgr_inpaint_batch"):
        img, mask = np.zeros((1, 4, 4, 3), np.uint8), np.ones((1, 4, 4), np.uint8)
        vs._check(vs.lib().vs_bgr_inpaint_batch(vs._p(img), 48, 1, 4, 4, 11, vs.FMT_BGR8, vs._p(mask), 16, 4, vs.MEM_HOST, None))     # rows shorter than 3 w
    s = vs.Stabilizer(device=0)
    assert s.get_inpaint() == 0
    s.set_inpaint(1)
    assert s.get_inpaint() == 1
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_inpaint(2)
    s.set_inpaint(0)
    assert s.get_inpaint() == 0
    with pytest.raises(vs.VsError, match="error -3"):               # a Lanczos2 handle
        vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2).set_inpaint(1)
    assert vs.Stabilizer(device=0, inpaint=1, border_fill=2).get_inpaint() == 1


# ---- the push-pull -----------------------------------------------------------------------------------------------------------
# (w, h): 129 x 65 -- the tail starts at level 1; 300 x 270 -- three full-size levels, then the tail; 64 x 4097 / 4097 x 64 -- the deepest
# pyramids on few texels (8 x 513 = 4104 texels at level 3: one more than the tail takes)
WINDOWS = [(1, 1), (2, 2), (1, 9), (9, 1), (63, 65), (129, 65), (300, 270), (64, 4097), (4097, 64)]
FORMATS = {"u8": (np.uint8, 255), "bgr10": (np.uint16, 1023), "bgr16": (np.uint16, 65535)}


def _fmt(vs, name):
    return {"u8": vs.FMT_BGR8, "bgr10": vs.FMT_BGR10, "bgr16": vs.FMT_BGR16_FULL}[name]


def _masks(rng, w, h):
    """random at 50 % kept; one kept pixel in a corner; one open pixel; a checkerboard; an open rim 5 pixels wide; an open hole of 130 x 130"""
    ys, xs = np.mgrid[0:h, 0:w]
    m = [(rng.random((h, w)) < 0.5).astype(np.uint8) * 255]
    corner = np.zeros((h, w), np.uint8)
    corner[h - 1, 0] = 1
    m.append(corner)
    one = np.full((h, w), 7, np.uint8)
    one[h // 2, w // 3] = 0
    m.append(one)
    m.append((((xs + ys) & 1) * 200).astype(np.uint8))
    rim = np.zeros((h, w), np.uint8)
    rim[5:-5, 5:-5] = 1
    m.append(rim)
    hole = np.ones((h, w), np.uint8)
    hole[max(h // 2 - 65, 0):h // 2 + 65, max(w // 2 - 65, 0):w // 2 + 65] = 0
    m.append(hole)
    return np.stack(m)


def _content(rng, n, w, h, dtype, maxv):
    # a ramp with noise on top: the roundings of both sentences matter somewhere, and the extremes occur
    ys, xs = np.mgrid[0:h, 0:w]
    ramp = ((xs * 3 + ys * 5) % (maxv + 1))[None, :, :, None]
    img = np.clip(ramp + rng.integers(-(maxv // 8), maxv // 8 + 1, (n, h, w, 3)), 0, maxv)
    img[:, ::7, ::5] = maxv
    img[:, 3::11, 2::3] = 0
    return img.astype(dtype)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("w,h", WINDOWS)
def test_inpaint_equals_the_rule(gpu_vs, w, h, fmt):
    vs = gpu_vs
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(w * 31 + h + maxv)
    masks = _masks(rng, w, h)
    imgs = _content(rng, len(masks), w, h, dtype, maxv)
    want = R.inpaint_batch(imgs, masks)
    got = vs.bgr_inpaint_batch(imgs, masks, fmt=_fmt(vs, fmt))
    for k in range(len(masks)):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    if w * h > 4:
        assert any(not np.array_equal(want[k], imgs[k]) for k in range(len(masks)))      # the test has teeth: open pixels changed


@pytest.mark.parametrize("fmt", ["u8", "bgr16"])
def test_pitched_strides_batches_and_junk(gpu_vs, fmt):
    vs = gpu_vs
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(17 + maxv)
    w, h = 131, 77
    masks = _masks(rng, w, h)[:3]
    masks[1] = 3                                                     # the middle frame is all-kept ...
    masks[2] = 0                                                     # ... and the last one all-open: both come back as they are
    imgs = _content(rng, 3, w, h, dtype, maxv)
    want = R.inpaint_batch(imgs, masks)
    assert np.array_equal(want[1], imgs[1]) and np.array_equal(want[2], imgs[2]) and not np.array_equal(want[0], imgs[0])
    assert np.array_equal(vs.bgr_inpaint_batch(imgs, masks, fmt=_fmt(vs, fmt)), want)
    guard = 0xA5 if dtype == np.uint8 else 0xA5A5
    got, raw = vs.bgr_inpaint_batch(imgs, masks, fmt=_fmt(vs, fmt), stride=3 * w + 7, mask_stride=w + 5, guard=guard)
    assert np.array_equal(got, want) and (raw[:, :, 3 * w:] == guard).all()
    # open pixels pre-filled with two different junk patterns: the same bytes
    keep = (masks != 0)[..., None]
    for junk in (0, maxv, None):
        other = np.where(keep, imgs, rng.integers(0, maxv + 1, imgs.shape).astype(dtype) if junk is None else junk).astype(dtype)
        other[2] = imgs[2]                                           # (an all-open window is left untouched: whatever it held)
        assert np.array_equal(vs.bgr_inpaint_batch(other, masks, fmt=_fmt(vs, fmt)), want), junk


@pytest.mark.parametrize("fmt", ["u8", "bgr10"])
def test_device_memory_inside_a_guard_band(gpu_vs, fmt):
    """image and mask in device memory with a guard band on all four sides (rows in front and behind, columns left and right): the band
    stays as it was"""
    import torch
    vs = gpu_vs
    dtype, maxv = FORMATS[fmt]
    rng = np.random.default_rng(23 + maxv)
    w, h, n, g = 300, 270, 2, 6
    masks = _masks(rng, w, h)[[0, 4]]
    imgs = _content(rng, n, w, h, dtype, maxv)
    want = R.inpaint_batch(imgs, masks)
    gv = 0x5A if dtype == np.uint8 else 0x5A5A
    big = np.full((n, h + 2 * g, (w + 2 * g) * 3), gv, dtype)
    big[:, g:g + h, 3 * g:3 * (g + w)] = imgs.reshape(n, h, 3 * w)
    mbig = np.full((n, h + 2 * g, w + 2 * g), 0x77, np.uint8)
    mbig[:, g:g + h, g:g + w] = masks
    tdt = torch.uint8 if dtype == np.uint8 else torch.int16
    dimg = torch.from_numpy(big.view(np.int16) if dtype != np.uint8 else big).cuda()
    dmask = torch.from_numpy(mbig).cuda()
    assert dimg.dtype == tdt
    torch.cuda.synchronize()
    stride, mstride, esz = (w + 2 * g) * 3, w + 2 * g, big.itemsize
    vs.bgr_inpaint_batch_device(dimg.data_ptr() + (g * stride + 3 * g) * esz, (h + 2 * g) * stride, n, w, h, stride, _fmt(vs, fmt),
                                dmask.data_ptr() + g * mstride + g, (h + 2 * g) * mstride, mstride)
    torch.cuda.synchronize()
    res = dimg.cpu().numpy().view(dtype)
    assert np.array_equal(res[:, g:g + h, 3 * g:3 * (g + w)].reshape(n, h, w, 3), want)
    res[:, g:g + h, 3 * g:3 * (g + w)] = gv
    assert (res == gv).all()
    assert np.array_equal(dmask.cpu().numpy(), mbig)
