"""vs_stabilizer_process_batch_ycbcr against its definition: vs_ycbcr_to_bgr_batch, vs_stabilizer_process_batch and vs_bgr_to_ycbcr_batch in
sequence, frame for frame and plane for plane, has_output and the output size included -- from host and from device memory, with other passes
on, with the output in another subsampling than the input, on an odd-sized clip, on a handle that was used through the BGR entry point before.
Planes of frames without an output keep their guard."""
import functools

import numpy as np
import pytest

import _ycbcr_ref as R

pytestmark = pytest.mark.gpu

GUARD = 0x5A
KW = dict(device=0, lag=4, crop_pixels=8, pyramid_min_width=10, pyramid_min_height=10)


@functools.lru_cache(maxsize=None)
def _clip(w, h, bits):
    from video_stabilizer_amd import synth
    return np.maximum(synth.make_clip(w, h, 24, seed=3, channels=3, bits=bits)[0], 1)


@functools.lru_cache(maxsize=None)
def _planes(w, h, bits, layout):
    """the clip as YCbCr planes of `layout`, by the restatement"""
    sub, _, mono = R.LAYOUTS[layout]
    return R.to_ycbcr(_clip(w, h, bits), sub, bits, mono)


def _by_the_three_calls(vs, planes, layout, out_layout, code, make):
    """the definition: ((y, cb, cr) of the frames that have an output, has_output)"""
    sub, inter, _ = R.LAYOUTS[layout]
    osub, ointer, omono = R.LAYOUTS[out_layout]
    bgr = vs.ycbcr_to_bgr_batch(*planes, sub=sub, fmt=code, interleaved=inter)
    out, has = make().process_batch(bgr, fmt=code)
    keep = np.array(has, bool)
    return vs.bgr_to_ycbcr_batch(out[keep], sub=osub, fmt=code, interleaved=ointer, mono=omono), has


def _check(got, has, want, want_has, guard):
    assert list(has) == list(want_has) and 0 < sum(has) < len(has)
    keep = np.array(has, bool)
    for g, r in zip(got, want):
        assert (g is None) == (r is None)
        if g is not None:
            assert g[keep].shape == r.shape and np.array_equal(g[keep], r)
            assert (g[~keep] == guard).all(), "planes of a frame without an output were written"


def _device_call(vs, stab, planes, layout, out_layout, code, w, h, crop):
    """process_batch_ycbcr_device on dense torch buffers -> ((y, cb, cr) of all n frames, has_output); the outputs start filled with the guard"""
    import torch
    sub, inter, mono = R.LAYOUTS[layout]
    osub, ointer, omono = R.LAYOUTS[out_layout]
    n = planes[0].shape[0]
    dtype = planes[0].dtype
    esz = dtype.itemsize
    guard = GUARD if esz == 1 else GUARD * 257
    up = (lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if esz == 2 else np.ascontiguousarray(a)).cuda())

    def build(y, cb, cr, ww, hh, s, il):
        cw, ch = R.chroma_shape(ww, hh, s)
        ty = up(y)
        if cb is None:
            return [ty], vs.ycbcr_planes(ty.data_ptr(), None, None, ww, 0, 1, s, ww * hh, 0)
        if il:
            pairs = np.stack((cb, cr) if il == "nv12" else (cr, cb), axis=3)
            tc = up(pairs)
            a, b = (tc.data_ptr(), tc.data_ptr() + esz) if il == "nv12" else (tc.data_ptr() + esz, tc.data_ptr())
            return [ty, tc], vs.ycbcr_planes(ty.data_ptr(), a, b, ww, 2 * cw, 2, s, ww * hh, 2 * cw * ch)
        tu, tv = up(cb), up(cr)
        return [ty, tu, tv], vs.ycbcr_planes(ty.data_ptr(), tu.data_ptr(), tv.data_ptr(), ww, cw, 1, s, ww * hh, cw * ch)
    ow, oh = w - 2 * crop, h - 2 * crop
    ocw, och = R.chroma_shape(ow, oh, osub)
    blank = (lambda *s: np.full(s, guard, dtype))
    tin, din = build(*planes, w, h, sub, inter)
    tout, dout = build(blank(n, oh, ow), None if omono else blank(n, och, ocw), None if omono else blank(n, och, ocw), ow, oh, osub, ointer)
    torch.cuda.synchronize()
    r, has, gw, gh = stab.process_batch_ycbcr_device(din, n, w, h, code, dout)
    torch.cuda.synchronize()
    assert (gw, gh) == (ow, oh) and r == sum(has)
    back = [t.cpu().numpy().view(dtype) for t in tout]
    if omono:
        return (back[0], None, None), has, guard
    if ointer:
        a, b = back[1][..., 0], back[1][..., 1]
        return ((back[0], a, b) if ointer == "nv12" else (back[0], b, a)), has, guard
    return tuple(back), has, guard


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_equals_the_three_public_calls(gpu_vs, fmt, layout):
    vs = gpu_vs
    code, dtype, bits = R.FORMATS[fmt]
    w, h = 160, 128
    planes = _planes(w, h, bits, layout)
    sub, inter, _ = R.LAYOUTS[layout]
    make = (lambda: vs.Stabilizer(**KW))
    want, want_has = _by_the_three_calls(vs, planes, layout, layout, code, make)
    guard = GUARD if dtype == np.uint8 else GUARD * 257
    got, has = make().process_batch_ycbcr(*planes, sub=sub, fmt=code, interleaved=inter, guard=guard)
    _check(got, has, want, want_has, guard)
    got, has, guard = _device_call(vs, make(), planes, layout, layout, code, w, h, KW["crop_pixels"])
    _check(got, has, want, want_has, guard)


def test_with_border_fill_denoise_and_lens_on(gpu_vs):
    vs = gpu_vs
    w, h = 160, 128
    lens = vs.lens_params(w, h, k1=-0.2, k2=0.05, zoom=1.05)
    make = (lambda: vs.Stabilizer(border_fill=3, denoise=2, lens=(lens, w, h), **dict(KW, crop_pixels=4)))
    for layout in ("i420", "nv12"):
        planes = _planes(w, h, 8, layout)
        sub, inter, _ = R.LAYOUTS[layout]
        want, want_has = _by_the_three_calls(vs, planes, layout, layout, vs.FMT_BGR8, make)
        got, has = make().process_batch_ycbcr(*planes, sub=sub, interleaved=inter, guard=GUARD)
        _check(got, has, want, want_has, GUARD)
        got, has, guard = _device_call(vs, make(), planes, layout, layout, vs.FMT_BGR8, w, h, 4)
        _check(got, has, want, want_has, guard)


@pytest.mark.parametrize("pair", [("i420", "i444"), ("nv12", "i422"), ("i444", "nv21"), ("i420", "mono")], ids="-".join)
def test_the_output_carries_its_own_subsampling(gpu_vs, pair):
    vs = gpu_vs
    layout, out_layout = pair
    w, h = 160, 128
    planes = _planes(w, h, 8, layout)
    sub, inter, _ = R.LAYOUTS[layout]
    osub, ointer, omono = R.LAYOUTS[out_layout]
    make = (lambda: vs.Stabilizer(**KW))
    want, want_has = _by_the_three_calls(vs, planes, layout, out_layout, vs.FMT_BGR8, make)
    got, has = make().process_batch_ycbcr(*planes, sub=sub, interleaved=inter, out_sub=osub, out_interleaved=ointer, out_mono=omono, guard=GUARD)
    _check(got, has, want, want_has, GUARD)
    got, has, guard = _device_call(vs, make(), planes, layout, out_layout, vs.FMT_BGR8, w, h, KW["crop_pixels"])
    _check(got, has, want, want_has, guard)


def test_an_odd_sized_clip(gpu_vs):
    """163 x 125: odd both ways, so the input's last chroma column and row hold one real pixel, and with crop 8 the output (147 x 109) is odd too.
    (Should the aligner refuse the size, the nearest odd size it takes is used: the loop below says which.)"""
    vs = gpu_vs
    make = (lambda: vs.Stabilizer(**KW))
    for w, h in ((163, 125), (161, 125), (165, 127), (161, 123)):
        try:
            make().process_batch(_clip(w, h, 8))
            break
        except vs.VsError:
            continue
    else:
        pytest.fail("the aligner refuses every odd size near 163 x 125")
    assert (w, h) == (163, 125), "the aligner refused 163 x 125; %d x %d is the nearest odd size it takes" % (w, h)
    for layout in ("i420", "nv12"):
        planes = _planes(w, h, 8, layout)
        sub, inter, _ = R.LAYOUTS[layout]
        want, want_has = _by_the_three_calls(vs, planes, layout, layout, vs.FMT_BGR8, make)
        got, has = make().process_batch_ycbcr(*planes, sub=sub, interleaved=inter, guard=GUARD)
        _check(got, has, want, want_has, GUARD)
        got, has, guard = _device_call(vs, make(), planes, layout, layout, vs.FMT_BGR8, w, h, KW["crop_pixels"])
        _check(got, has, want, want_has, guard)


def test_a_handle_used_through_the_bgr_entry_point_first(gpu_vs):
    """process_batch, reset, process_batch_ycbcr on one handle gives what a fresh handle gives; and the other way round"""
    vs = gpu_vs
    w, h = 160, 128
    planes = _planes(w, h, 8, "i420")
    bgr = vs.ycbcr_to_bgr_batch(*planes)
    fresh, fresh_has = vs.Stabilizer(**KW).process_batch_ycbcr(*planes, guard=GUARD)
    fresh_bgr, _ = vs.Stabilizer(**KW).process_batch(bgr)
    s = vs.Stabilizer(**KW)
    s.process_batch(bgr[:17])
    s.reset()
    got, has = s.process_batch_ycbcr(*planes, guard=GUARD)
    assert has == fresh_has and all(np.array_equal(g, r) for g, r in zip(got, fresh))
    s.reset()
    again, has2 = s.process_batch(bgr)
    assert has2 == fresh_has and np.array_equal(again, fresh_bgr)
