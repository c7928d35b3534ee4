"""The fill's seam blend on the GPU (include/vs_amd.h: vs_bgr_channel_sums_batch, vs_bgr_image_warp_fill_blend_batch,
vs_stabilizer_set_fill_blend) against the rule's reference (tests/_fill_blend_ref.py: numpy on top of the CPU oracle).  Kernel level:
np.array_equal, on device memory inside guard bands (tests/_fill_blend_direct.py).  Engine against the oracle's engine model: the fill tests' gate
(tests/test_fill_gpu.py: at most 1e-4 of the samples differ, the two engines' transforms agree to about 1e-12 but not bit for bit); against the
model fed with the engine's OWN transforms (they agree exactly): np.array_equal.  Engine routes against each other: np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _engine_model as EM
import _fill_blend_direct as D
import _fill_blend_ref as B
import _fill_ref as R
import _hostile_maps as HM
from _stab_routes import assert_every_route_equals, frame_by_frame, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240
SIZES = [(1, 1), (2, 2), (3, 5), (63, 17), (65, 16), (300, 270)]
KINDS = [(8, 255, np.uint8), (10, 1023, np.uint16), (16, 65535, np.uint16)]
SETTINGS = [(f, m) for f in (0, 1, 4, 6) for m in (0, 1)]


def _ot(O, maps):
    return [[O.Transform.of(*t) for t in row] for row in maps]


# ---- channel sums ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10", "bgr12", "bgr16"])
def test_channel_sums_equal_numpy(gpu_vs, fmt):
    """every size, dense / pitched rows and an odd base address, so that the dword variant (base and pitch on dwords) and the per-sample variant
    both run; containers that hold samples above the format's maximum (no clamp)"""
    vs = gpu_vs
    code, dtype, bits = HM.FORMATS[fmt]
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(bits)
    for w, h in SIZES:
        n = 3
        src = rng.integers(0, 1 << bits, (n, h, w, 3)).astype(dtype)
        if bits not in (8, 16):
            src[rng.random(src.shape) < 0.1] = 65535                  # above the format's maximum
            src[0, 0, 0] = (65535, 1 << bits, 65535)
        want = B.channel_sums(src)
        assert bits in (8, 16) or (want > np.uint64(((1 << bits) - 1) * w * h)).any()
        on_dwords = (3 * w + (-3 * w) % 4)                            # the next pitch that keeps every row on a dword (in elements, both sizes)
        for ss, base in ((None, 0), (on_dwords + 4, 0), (3 * w + 1, 0), (3 * w + 3, 0), (None, 1), (on_dwords, 3)):
            got = D.dev_sums(vs, src, code, ss=ss, base=base)
            assert np.array_equal(got, want), (w, h, ss, base, got.tolist(), want.tolist())
        assert np.array_equal(vs.channel_sums_batch(src, fmt=code), want)                     # host memory
        assert np.array_equal(vs.channel_sums_batch(src, fmt=code, src_stride=3 * w + 5), want)
    if esz == 1:
        assert (3 * 63 + 1) % 4 and (3 * 300 + 4) % 4 == 0            # the pitches above are on and off dwords


def test_channel_sums_of_a_full_16_bit_frame_do_not_wrap(gpu_vs):
    """a 300 x 270 frame of 65535: every wave's share, every lane's accumulator at its largest"""
    src = np.full((1, 270, 300, 3), 65535, np.uint16)
    assert D.dev_sums(gpu_vs, src, HM.FORMATS["bgr16"][0]).tolist() == [[65535 * 300 * 270] * 3]
    assert D.dev_sums(gpu_vs, src, HM.FORMATS["bgr16"][0], ss=901).tolist() == [[65535 * 300 * 270] * 3]


# ---- the blend kernel ------------------------------------------------------------------------------------------------------------------------
def _case(rng, w, h, dtype, maxv, n_cand, n_src=5, n_out=2):
    src = D.frames(rng, n_src, w, h, dtype, maxv)
    maps = [[HM._rot(rng, w, h, big=True) for _ in range(n_cand)] for _ in range(n_out)]
    # output 0: a small correction as candidate 0 (a rim a few pixels wide: the case the engine produces)
    maps[0][0] = (0.01, -0.015, 0.04 * w, -0.03 * h)
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    if n_cand >= 3:
        cf[1, n_cand - 1] = -1
    return src, cf, maps


# two candidates at every size; sixteen at one small and one multi-block size
SHAPE_CANDS = [(s, 2) for s in SIZES + [(520, 70)]] + [((63, 17), 16), ((300, 270), 16)]


@pytest.mark.parametrize("shape,n_cand", SHAPE_CANDS, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "c%d" % v)
@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10", "bgr16"])
def test_blend_equals_the_rule(gpu_vs, oracle, bits, maxv, dtype, shape, n_cand):
    """feather x match crossed, both borders (alternating over the settings), rotations to +-0.5 rad with zooms 0.6 .. 1.6; at 300 x 270 (2 x 2
    blocks) and 520 x 70 the band crosses block and strip seams"""
    vs, O = gpu_vs, oracle
    w, h = shape
    rng = np.random.default_rng(1000 * bits + 7 * w + h + n_cand)
    src, cf, maps = _case(rng, w, h, dtype, maxv, n_cand)
    sums = B.channel_sums(src)
    ct = _ot(O, maps)
    changed = 0
    for i, (feather, match) in enumerate(SETTINGS):
        border = (vs.BORDER_CONSTANT, vs.BORDER_CLAMP)[i % 2]
        want = B.blend_batch(O, src, cf, ct, sums, feather, match, border, maxv)
        got = D.dev_blend(vs, src, cf, maps, sums if (match or i % 4 == 2) else None, feather, match, border=border, maxv=maxv,
                          ss=3 * w + (7 if i % 3 == 0 else 0), ds=3 * w + (5 if i % 3 == 1 else 0))
        assert np.array_equal(got, want), (feather, match, border, int((got != want).sum()))
        changed += int((want != R.fill_batch(O, src, cf, ct, border, maxv)).sum())
    if min(w, h) >= 16:
        assert changed > 0                                           # the switches did something
        roi = (5, 3, w - 11, h - 7)
        want = B.blend_batch(O, src, cf, ct, sums, 4, 1, vs.BORDER_CONSTANT, maxv, roi=roi)
        got = D.dev_blend(vs, src, cf, maps, sums, 4, 1, roi=roi, maxv=maxv, ds=3 * roi[2] + 2)
        assert np.array_equal(got, want), ("roi", int((got != want).sum()))
        host = vs.bgr_image_warp_fill_blend_batch(src, cf, [[vs.Transform.of(*t) for t in row] for row in maps], sums, 4, 1, roi=roi, max_value=maxv)
        assert np.array_equal(host, want)                            # host memory


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10", "bgr16"])
def test_every_covered_pixel_in_the_band(gpu_vs, oracle, bits, maxv, dtype):
    """40 x 30 with feather 6: no pixel is 64 source pixels inside the frame (premise), so no block and no strip is deep inside"""
    vs, O = gpu_vs, oracle
    w, h = 40, 30
    rng = np.random.default_rng(bits)
    src, cf, maps = _case(rng, w, h, dtype, maxv, 3, n_out=3)
    maps[2][0] = (0.0, 0.0, 0.0, 0.0)
    sums = B.channel_sums(src)
    ct = _ot(O, maps)
    for row in ct:
        kk, cov = B.plain_weight(O, row[0], w, h, 6)
        assert cov.any() and (kk[cov] < (32 << 6)).all()
    for match in (0, 1):
        for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
            want = B.blend_batch(O, src, cf, ct, sums, 6, match, border, maxv)
            got = D.dev_blend(vs, src, cf, maps, sums, 6, match, border=border, maxv=maxv)
            assert np.array_equal(got, want), (match, border, int((got != want).sum()))
    assert not np.array_equal(want, B.blend_batch(O, src, cf, ct, sums, 0, 1, vs.BORDER_CLAMP, maxv))


def test_1080p(gpu_vs, oracle):
    from video_stabilizer_amd import synth
    vs, O = gpu_vs, oracle
    frames, _ = synth.make_clip(1920, 1080, 3, seed=21, channels=3, jitter_t=12.0)
    frames[1] = (frames[1].astype(np.int64) * 9 // 10).astype(np.uint8)
    maps = [[(0.004, -0.006, 23.5, -17.25), (0.006, -0.003, 40.0, -2.0), (0.001, -0.008, 5.5, -30.0)]]
    cf = np.array([[0, 1, 2]], np.int32)
    sums = B.channel_sums(frames)
    want = B.blend_batch(O, frames, cf, _ot(O, maps), sums, 4, 1, O.BORDER_CONSTANT, 255)
    got = D.dev_blend(vs, frames, cf, maps, sums, 4, 1, maxv=255)
    assert np.array_equal(got, want)
    assert np.array_equal(D.dev_sums(vs, frames, vs.FMT_BGR8), sums)


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10", "bgr16"])
def test_both_switches_off_is_the_fill_call(gpu_vs, oracle, bits, maxv, dtype):
    vs, O = gpu_vs, oracle
    w, h = 203, 149
    rng = np.random.default_rng(bits + 50)
    src, cf, maps = _case(rng, w, h, dtype, maxv, 5, n_out=4)
    gct = [[vs.Transform.of(*t) for t in row] for row in maps]
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        for roi in (None, (13, 9, 131, 77)):
            a = vs.bgr_image_warp_fill_batch(src, cf, gct, roi=roi, border=border, max_value=maxv)
            assert np.array_equal(vs.bgr_image_warp_fill_blend_batch(src, cf, gct, None, 0, 0, roi=roi, border=border, max_value=maxv), a)
            assert np.array_equal(D.dev_blend(vs, src, cf, maps, B.channel_sums(src), 0, 0, roi=roi, border=border, maxv=maxv), a)
    # one candidate, or no later candidate: the plain ROI warp with any setting
    own = [row[0] for row in gct]
    plain = vs.bgr_image_warp_roi_batch(src[:4], own, (0, 0, w, h), mode=vs.WARP_BILINEAR_CV, border=vs.BORDER_CONSTANT, max_value=maxv)
    idx = np.arange(4, dtype=np.int32)[:, None]
    assert np.array_equal(vs.bgr_image_warp_fill_blend_batch(src, idx, [[t] for t in own], B.channel_sums(src), 6, 1, max_value=maxv), plain)
    cut = np.concatenate([idx, np.full((4, 4), -1, np.int32)], axis=1)
    gct0 = [[row[0]] + row[1:] for row in gct]
    assert np.array_equal(vs.bgr_image_warp_fill_blend_batch(src, cut, gct0, B.channel_sums(src), 6, 1, max_value=maxv), plain)
    # identical frames under identity maps: bit for bit
    same = np.stack([src[0]] * 3)
    ident = [[vs.Transform.of()] * 3]
    got = vs.bgr_image_warp_fill_blend_batch(same, [[0, 1, 2]], ident, B.channel_sums(same), 5, 1, max_value=maxv)
    assert np.array_equal(got, vs.bgr_image_warp_roi_batch(same[:1], ident[0][:1], (0, 0, w, h), mode=vs.WARP_BILINEAR_CV, border=vs.BORDER_CONSTANT, max_value=maxv))


def test_argument_errors(gpu_vs):
    vs = gpu_vs
    src = np.zeros((3, 32, 48, 3), np.uint8)
    sums = np.zeros((3, 3), np.uint64)
    t = vs.Transform.of(0, 0, 3, 2)
    assert vs.bgr_image_warp_fill_blend_batch(src, [[0, 1]], [[t, t]], sums, 6, 1).shape == (1, 32, 48, 3)
    for feather, match in ((-1, 0), (7, 0), (0, 2), (0, -1), (3, 5)):
        with pytest.raises(vs.VsError, match="error -1"):
            vs.bgr_image_warp_fill_blend_batch(src, [[0, 1]], [[t, t]], sums, feather, match)
    with pytest.raises(vs.VsError, match="error -1"):               # match without sums
        vs.bgr_image_warp_fill_blend_batch(src, [[0, 1]], [[t, t]], None, 0, 1)
    assert vs.bgr_image_warp_fill_blend_batch(src, [[0, 1]], [[t, t]], None, 3, 0).shape == (1, 32, 48, 3)
    with pytest.raises(vs.VsError, match="error -1"):               # the fill's own checks
        vs.bgr_image_warp_fill_blend_batch(src, [[0, 3]], [[t, t]], sums, 1, 1)
    with pytest.raises(vs.VsError, match="error -1"):
        vs.bgr_image_warp_fill_blend_batch(src, [[0] * 17], [[t] * 17], sums, 1, 1)
    idx = np.array([[0, 1]], np.int32)
    arr = (vs.Transform * 2)(t, t)
    out = np.zeros((1, 32, 48, 3), np.uint8)
    r = vs.lib().vs_bgr_image_warp_fill_blend_batch(vs._p(src), 32 * 48 * 3, 3, 48, 32, 48 * 3, 3, 8, 1, 2, idx.ctypes.data_as(C.POINTER(C.c_int32)), arr,
                                                    vs._p(sums), None, vs.BORDER_CONSTANT, 255, 0, 0, 48, 32, vs._p(out), 32 * 48 * 3, 48 * 3, vs.MEM_HOST, None)
    assert r == -1                                                   # params are required
    with pytest.raises(vs.VsError, match="error -1"):               # sums: a gray format
        vs.channel_sums_batch(src, fmt=vs.FMT_GRAY8)
    r = vs.lib().vs_bgr_channel_sums_batch(vs._p(src), 0, 1, 32768, 1, 3 * 32768, vs.FMT_BGR8, vs._p(sums), vs.MEM_HOST, None)
    assert r == -3                                                   # beyond 32767: unsupported, as the fill
    s = vs.Stabilizer(device=0, lag=6)
    assert s.fill_blend() == (0, 0)
    for feather, match in ((-1, 0), (7, 1), (0, 2)):
        with pytest.raises(vs.VsError, match="error -1"):
            s.set_fill_blend(feather, match)
    s.set_fill_blend(6, 1)
    assert s.fill_blend() == (6, 1)
    assert vs.lib().vs_stabilizer_set_fill_blend(s.h, None) == 0     # NULL: off
    assert s.fill_blend() == (0, 0)
    lz = vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2)
    with pytest.raises(vs.VsError, match="error -3"):               # a Lanczos2 handle
        lz.set_fill_blend(2, 0)
    assert vs.Stabilizer(device=0, border_fill=3, fill_blend=(2, 1)).fill_blend() == (2, 1)


# ---- the engine --------------------------------------------------------------------------------------------------------------------------------
def _clip(n, seed, bits=8, w=W, h=H, drift=True, **kw):
    """a synthetic clip whose exposure drifts from frame to frame (+-10 %)"""
    from video_stabilizer_amd import synth
    c = synth.make_clip(w, h, n, seed=seed, channels=3, bits=bits, **kw)[0]
    if not drift:
        return c
    g = 1.0 + 0.1 * np.sin(2 * np.pi * np.arange(n) / 7.0 + seed)
    maxv = 255 if bits == 8 else (1 << bits) - 1
    return np.clip(np.rint(c.astype(np.float64) * g[:, None, None, None]), 0, maxv).astype(c.dtype)


def _cut_clip(bits):
    """40 frames with a three-frame scene cut in the middle: the alignment fails there (asserted where the model is run)"""
    a = _clip(30, 5, bits)
    return np.concatenate([a[:14], _clip(3, 77, bits), a[14:]])


def _own_transform_model(vs, O, frames, ahead, feather, match, maxv, plain=None, **kw):
    """the engine frame by frame, and the rule applied with the engine's OWN measurements and corrections (vs_stabilizer_state after every frame,
    composed with the library's vs_transform_compose / _inverse as the engine composes them) -> (engine outputs, modelled outputs).  plain: {k: the
    plain warp of output k} where candidate 0 is not the input frame (deblur / denoise on; crop 0)"""
    st = vs.Stabilizer(device=0, border_fill=ahead, fill_blend=(feather, match), **kw)
    lag, crop = st.params.lag, max(st.params.crop_pixels, 0)
    n, h, w, _ = frames.shape
    meas, succ, due, got = [], [], {}, {}
    for i, f in enumerate(frames):
        o = st.process(f)
        m, a, s = st.state()
        meas.append(m)
        succ.append(s)
        if o is not None:
            due[i - lag], got[i - lag] = a, o
    sums = B.channel_sums(frames)
    want = {}
    for k, acc in due.items():
        cf, ct = EM.fill_candidates(vs, k, ahead, meas, succ, vs.t_inverse(acc))
        want[k] = B.blend_frame(O, frames, cf, [O.Transform.of(*t.tup()) for t in ct], sums, feather, match, st.params.warp_border, maxv,
                                (crop, crop, w - 2 * crop, h - 2 * crop), plain=None if plain is None else plain[k])
    return got, want


@pytest.mark.parametrize("crop", [0, 32])
@pytest.mark.parametrize("bits", [8, 10])
def test_engine_equals_the_engine_model(gpu_vs, oracle, bits, crop):
    vs, O = gpu_vs, oracle
    frames = _cut_clip(bits)
    maxv = 255 if bits == 8 else 1023
    kw = dict(lag=6, crop_pixels=crop)
    model = EM.engine_model(O, frames, fill=4, blend=(4, 1), want_masks=True, **kw)
    st = O.Stabilizer(**kw)
    succ = []
    for f in frames:
        st.process(f)
        succ.append(st.state()[2])
    assert not all(succ[1:]), "the scene cut no longer makes the alignment fail: the test input has to change"
    got, own = _own_transform_model(vs, O, frames, 4, 4, 1, maxv, **kw)
    assert sorted(got) == sorted(model.outs) == sorted(own)
    diff = total = filled = banded = 0
    for k, want in model.outs.items():
        cov0, still_open, band = model.masks[k]
        diff += int((got[k] != want).sum())
        total += want.size
        filled += int((~cov0 & ~still_open).sum())
        banded += int(band.sum())
    print("%d-bit crop %d: %d of %d samples differ (share %.3g), %d pixels filled, %d blended" % (bits, crop, diff, total, diff / total, filled, banded))
    if crop == 0:
        assert filled > 0 and banded > 0
    assert diff <= 1e-4 * total
    # where the transforms agree (the engine's own): bit for bit
    bad = [k for k in own if not np.array_equal(got[k], own[k])]
    assert not bad, bad
    plain = frame_by_frame(vs.Stabilizer(device=0, border_fill=4, **kw), frames)
    if crop == 0:
        assert any(not np.array_equal(plain[k], got[k]) for k in got)


@pytest.mark.parametrize("bits", [8, 10])
def test_every_route_gives_the_same_frames(gpu_vs, bits):
    """process frame by frame == process_batch (one call; split calls) == device memory == process_clips, with the blend on; a scene cut in the middle"""
    import torch
    vs = gpu_vs
    frames = _cut_clip(bits)
    n = len(frames)
    kw = dict(device=0, lag=6, crop_pixels=8, border_fill=4, fill_blend=(3, 1))
    ref = frame_by_frame(vs.Stabilizer(**kw), frames)
    plain = frame_by_frame(vs.Stabilizer(device=0, lag=6, crop_pixels=8, border_fill=4), frames)
    assert any(not np.array_equal(ref[k], plain[k]) for k in ref)
    assert_every_route_equals(vs, kw, frames, ref, (3, 1, 9, 2, 11, n - 26))         # (split calls: queued frames keep their sums between the calls)
    fmt = vs.FMT_BGR8 if bits == 8 else vs.FMT_BGR10
    # process_clips: two clips, host and device memory
    half = n // 2
    two = np.concatenate([frames[:half], frames[:half]])
    one = frame_by_frame(vs.Stabilizer(**kw), frames[:half])
    out, has = vs.Stabilizer(**kw).process_clips(two, 2)
    dev = torch.from_numpy(two.view(np.int16) if bits != 8 else two).cuda()
    dout = torch.zeros((2 * half, H - 16, W - 16, 3), dtype=dev.dtype, device="cuda")
    r, dhas = vs.Stabilizer(**kw).process_clips_device(dev.data_ptr(), 2, half, W, H, fmt, dout.data_ptr())
    torch.cuda.synchronize()
    dres = dout.cpu().numpy().view(frames.dtype)
    assert list(has) == list(dhas)
    for c in range(2):
        for i in range(half):
            assert bool(has[c * half + i]) == (i - 6 in one)
            if has[c * half + i]:
                assert np.array_equal(out[c * half + i], one[i - 6]), (c, i)
                assert np.array_equal(dres[c * half + i], one[i - 6]), (c, i)


def test_chunked_and_pipelined_batches(gpu_vs, monkeypatch):
    """a device-resident clip long enough for the time chunks (warps and the gain kernel on their own stream, behind the sums of the ingest stream)
    and a host batch long enough for the upload / compute / download pipeline, against short process_batch calls"""
    import torch
    vs = gpu_vs
    w, h, n = 480, 360, 260
    frames = _clip(n, 9, w=w, h=h, pan=0.2)
    monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(37 * w * h * 3))
    kw = dict(device=0, lag=6, crop_pixels=0, border_fill=4, fill_blend=(4, 1))
    st = vs.Stabilizer(**kw)
    ref = np.zeros_like(frames)
    ref_has = []
    for p in range(0, n, 20):
        o, hs = st.process_batch(frames[p:p + 20])
        ref[p:p + 20] = o
        ref_has += hs
    plain, _ = vs.Stabilizer(device=0, lag=6, crop_pixels=0, border_fill=4).process_batch(frames[:40])
    assert not np.array_equal(plain, ref[:40])
    out, has = vs.Stabilizer(**kw).process_batch(frames)
    assert has == ref_has and np.array_equal(out, ref)
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    r, hs = vs.Stabilizer(**kw).process_batch_device(dev.data_ptr(), n, w, h, vs.FMT_BGR8, dout.data_ptr())
    torch.cuda.synchronize()
    assert hs == ref_has and np.array_equal(dout.cpu().numpy(), ref)


def test_with_deblur_and_denoise_on(gpu_vs, oracle):
    """the order stays deblur, denoise, warp, fill; the sums are the ORIGINAL frames', the candidates the original frames: the rule with the plain
    value taken from the handle without the fill (the warp of the deblurred, denoised frame) and everything else from the input frames, bit for bit;
    every route agrees; both switches off is the handle without the call"""
    vs, O = gpu_vs, oracle
    frames = _cut_clip(8)
    base = dict(device=0, lag=6, crop_pixels=0, border_fill=4, deblur=3, denoise=3)
    plain = frame_by_frame(vs.Stabilizer(**base), frames)
    off = vs.Stabilizer(**base)
    off.set_fill_blend(0, 0)
    got = frame_by_frame(off, frames)
    assert all(np.array_equal(got[k], plain[k]) for k in plain)
    nofill = frame_by_frame(vs.Stabilizer(device=0, lag=6, crop_pixels=0, deblur=3, denoise=3), frames)
    for blend in ((4, 0), (4, 1), (0, 1)):
        ref = frame_by_frame(vs.Stabilizer(fill_blend=blend, **base), frames)
        assert any(not np.array_equal(ref[k], plain[k]) for k in ref), blend
        out, has = vs.Stabilizer(fill_blend=blend, **base).process_batch(frames)
        for i, hh in enumerate(has):
            if hh:
                assert np.array_equal(out[i], ref[i - 6]), (blend, i)
        st = vs.Stabilizer(fill_blend=blend, **base)
        pos = 0
        for m in (5, 2, 13, len(frames) - 20):
            o, hs = st.process_batch(frames[pos:pos + m])
            for i, hh in enumerate(hs):
                if hh:
                    assert np.array_equal(o[i], ref[pos + i - 6]), (blend, pos, i)
            pos += m
        got, own = _own_transform_model(vs, O, frames, 4, blend[0], blend[1], 255, plain=nofill, lag=6, crop_pixels=0, deblur=3, denoise=3)
        assert sorted(got) == sorted(ref) and all(np.array_equal(got[k], ref[k]) for k in ref)
        bad = [k for k in own if not np.array_equal(got[k], own[k])]
        assert not bad, (blend, bad)


def test_switching_on_mid_clip_equals_on_from_the_start(gpu_vs):
    vs = gpu_vs
    frames = _clip(34, 5)
    kw = dict(device=0, lag=6, crop_pixels=0, border_fill=4)
    a = vs.Stabilizer(**kw)
    b = vs.Stabilizer(fill_blend=(3, 1), **kw)
    c = vs.Stabilizer(**kw)
    seen_diff = False
    for i, f in enumerate(frames):
        if i == 11:                                                  # six frames are queued without sums: they are summed at the next call
            a.set_fill_blend(3, 1)
        if i == 24:
            a.set_fill_blend(0, 0)
        oa, ob, oc = a.process(f), b.process(f), c.process(f)
        if oa is None:
            assert ob is None and oc is None
            continue
        if 11 <= i < 24:
            assert np.array_equal(oa, ob), i                         # on from the start
            seen_diff |= not np.array_equal(oa, oc)
        else:
            assert np.array_equal(oa, oc), i                         # off after on, and before: never on
    assert seen_diff
    # the same with batches: switched on between two calls
    a = vs.Stabilizer(**kw)
    o1, h1 = a.process_batch(frames[:13])
    a.set_fill_blend(3, 1)
    o2, h2 = a.process_batch(frames[13:])
    ref, rh = vs.Stabilizer(fill_blend=(3, 1), **kw).process_batch(frames)
    assert list(h2) == list(rh[13:])
    for i, hh in enumerate(h2):
        if hh:
            assert np.array_equal(o2[i], ref[13 + i]), i


@pytest.mark.parametrize("throwing", [False, True])
def test_blended_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    """(the plain fill's walk fails 17 allocations at least on this call: tests/test_fill_gpu.py; the sums' block is one more)"""
    vs = gpu_vs
    frames = _clip(16, 7)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    n = walk(vs, lambda: vs.Stabilizer(device=0, lag=4, smoother_memory=2, crop_pixels=8, border_fill=3, fill_blend=(3, 1)), call, 18, throwing)
    print("blended process_batch: %d allocations failed one by one (%s)" % (n, "throwing" if throwing else "error code"))


def test_video_test_blend_writes_what_the_library_returns(gpu_vs, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    frames = _clip(40, 77)
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    exe = os.path.join(ROOT, "apps", "bin", "vs_video_test")
    r = subprocess.run([exe, str(d), str(tmp_path / "out"), "--crop", "0", "--fill", "4", "--fill-feather", "4", "--fill-match", "--chunk", "13"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = gpu_vs.Stabilizer(device=0, crop_pixels=0, border_fill=4, fill_blend=(4, 1))
    want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_" + raw.name), np.uint8).reshape(-1, H, W, 3)
    assert np.array_equal(got, want)
    plain = gpu_vs.Stabilizer(device=0, crop_pixels=0, border_fill=4)
    assert not np.array_equal(want, np.stack([o for o in (plain.process(f) for f in frames) if o is not None]))
    r = subprocess.run([exe, str(d), str(tmp_path / "out2"), "--fill-feather", "9", "--fill", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "vs_stabilizer_set_fill_blend" in r.stderr
