"""Temporal denoise on the GPU (include/vs_amd.h: vs_bgr_denoise_batch, vs_stabilizer_set_denoise) against the rule's restatement
(tests/_denoise_ref.py).  Kernel level: np.array_equal -- the rule fixes every bit.  Engine against the kernel-level calls fed with candidates
built here from a capi.Aligner's measurements: np.array_equal (the same host algebra, the same doubles).  Engine against the engine model on
the CPU oracle's transforms: the two engines' transforms agree to about 1e-12 but not bit for bit and a table entry can flip on that, so the
gate there is DESIGN section 14's share -- at most 1e-4 of the samples differ.  Engine routes against each other: np.array_equal.
Every case asserts its premise on the CPU reference before it looks at the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _denoise_ref as R
import _engine_model as EM
from _stab_routes import assert_every_route_equals, frame_by_frame, walk
from test_deblur_gpu import _plain_clip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240
FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}
# tile and strip seams of both instantiations (64 x 32 tiles of 8-row strips; 256 x 16 tiles of 4-row strips for widths that are multiples of
# 4) and frames smaller than a wave
SHAPES = [(1, 1), (1, 5), (3, 1), (2, 2), (4, 17), (8, 16), (63, 15), (65, 65), (67, 129), (64, 16), (256, 64), (260, 65), (516, 17)]
KINDS = ("noise", "constant", "checker")
STRENGTHS = (1, 24, 255)


def _o(O, t):
    return O.Transform.of(*t.tup())


def _content(rng, kind, n, w, h, dtype, maxv):
    """noise: one smooth picture under fresh noise of +- 8 levels per frame (the candidates agree with the target: they take part);
    constant: the format's maximum; checker: a one-pixel checkerboard of 0 and the maximum (interpolated samples take every value between)"""
    scale = (maxv + 1) // 256
    if kind == "noise":
        yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
        base = (70 + (xx * 3 + yy * 2) % 120 + 10 * cc) * scale
        return np.clip(base[None] + rng.integers(-8 * scale, 8 * scale + 1, (n, h, w, 3)), 0, maxv).astype(dtype)
    if kind == "constant":
        return np.full((n, h, w, 3), maxv, dtype)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.broadcast_to((((xx + yy) & 1) * maxv)[None, :, :, None], (n, h, w, 3)).astype(dtype)


def _cand_lists(vs, rng, n_out, n_cand, n_src, w, h):
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    ct = []
    for o in range(n_out):
        row = [vs.Transform.of(*rng.uniform(-1, 1, 4))]               # (candidate 0's transform is ignored)
        for c in range(1, n_cand):
            row.append(vs.Transform.of(rng.uniform(-0.01, 0.01), rng.uniform(-0.02, 0.02), rng.uniform(-2.5, 2.5), rng.uniform(-2.5, 2.5)))
        if n_cand >= 3:
            row[2] = vs.Transform.of(0.0, 0.0, 3.0 * w + 7, -2.0 * h - 5)     # a map that leaves the frame altogether
        if n_cand >= 4:
            row[3] = vs.Transform.of(0.0, 0.0, 1.0, -1.0)             # an integer shift: zero fraction
        if n_cand >= 5 and o % 2 == 1:
            cf[o, 4] = -1                                            # the list ends early
        ct.append(row)
    return cf, ct


@pytest.mark.parametrize("n_cand", [2, 16])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_denoise_batch_equals_the_rule(gpu_vs, oracle, fmt, n_cand):
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(1000 * bits + n_cand)
    guard = 0x5A if bits == 8 else 0x5A5A
    n_src, n_out = 4, 2
    blended = 0
    for si, (w, h) in enumerate(SHAPES):
        cf, ct = _cand_lists(vs, rng, n_out, n_cand, n_src, w, h)
        oct_ = [[_o(O, t) for t in row] for row in ct]
        for ki, kind in enumerate(KINDS):
            strength = STRENGTHS[(si + ki) % 3]
            p = vs.denoise_params(strength=strength)
            src = _content(rng, kind, n_src, w, h, dtype, maxv)
            want = R.denoise_batch(O, src, cf, oct_, bits, maxv, strength)
            assert (np.abs(want.astype(np.int64) - src[cf[:, 0]].astype(np.int64)) < (strength << (bits - 8))).all()      # the ghost bound
            blended += int((want != src[cf[:, 0]]).sum())
            got = vs.denoise_batch(src, cf, ct, params=p, fmt=code)
            assert np.array_equal(got, want), (w, h, kind, strength, int((got != want).sum()))
            if kind != "noise":
                continue
            # pitched rows on both sides (odd: the four-pixel kernel's group falls back to the per-sample one), the destination inside a
            # guard band that must stay untouched; then rows that start on dwords
            for ss, ds in ((3 * w + 7, 3 * w + 5), (3 * w + 8, 3 * w + 4)):
                res, padded = vs.denoise_batch(src, cf, ct, params=p, fmt=code, src_stride=ss, dst_stride=ds, guard=guard)
                assert np.array_equal(res, want), (w, h, ss, ds)
                assert (padded[:, :, 3 * w:] == guard).all()
    assert blended > 10000                                           # the comparison was about blended samples


def test_default_parameters_one_candidate_and_identical_frames(gpu_vs, oracle):
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(3)
    w, h = 260, 75
    src = _content(rng, "noise", 3, w, h, np.uint8, 255)
    ident = vs.Transform.of()
    # NULL parameters are strength 24
    want = R.denoise_frame(O, src, [0, 1, 2], [O.Transform.of()] * 3, 8, 255, 24)
    assert not np.array_equal(want, src[0])
    assert np.array_equal(vs.denoise_batch(src, [[0, 1, 2]], [[ident] * 3])[0], want)
    # (a) one candidate, a list that ends at once, candidates outside the frame: a copy (both instantiations: the odd pitch falls back)
    far = vs.Transform.of(0, 0, 1000, 0)
    for kw in (dict(), dict(src_stride=3 * w + 1, dst_stride=3 * w + 3)):
        assert np.array_equal(vs.denoise_batch(src, [[1]], [[ident]], **kw)[0], src[1])
        assert np.array_equal(vs.denoise_batch(src, [[1, -1, 2]], [[ident] * 3], **kw)[0], src[1])
        assert np.array_equal(vs.denoise_batch(src, [[1, 0, 2]], [[ident, far, far]], **kw)[0], src[1])
        # (b) identical frames under identity maps
        assert np.array_equal(vs.denoise_batch(src, [[2, 2, 2, 2]], [[ident] * 4], **kw)[0], src[2])


def test_device_memory_equals_host_memory(gpu_vs, oracle):
    import torch
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(5)
    w, h, n_src, n_out, n_cand = 132, 50, 6, 40, 5                   # (40 outputs x 5 candidates: more than a kernel-argument block carries)
    src = _content(rng, "noise", n_src, w, h, np.uint8, 255)
    cf, ct = _cand_lists(vs, rng, n_out, n_cand, n_src, w, h)
    want = R.denoise_batch(O, src, cf, [[_o(O, t) for t in row] for row in ct], 8, 255, 24)
    assert np.array_equal(vs.denoise_batch(src, cf, ct), want)
    dsrc = torch.from_numpy(src).cuda()
    dout = torch.zeros((n_out, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vs.denoise_batch_device(dsrc.data_ptr(), h * w * 3, n_src, w, h, w * 3, vs.FMT_BGR8, cf, ct, dout.data_ptr(), h * w * 3, w * 3)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), want)


def test_argument_errors_and_the_handle_s_boundary(gpu_vs):
    vs = gpu_vs
    src = np.zeros((3, 32, 48, 3), np.uint8)
    t = vs.Transform.of(0, 0, 3, 2)
    assert vs.denoise_batch(src, [[0, 1]], [[t, t]]).shape == (1, 32, 48, 3)
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 0
        vs.denoise_batch(src, np.zeros((1, 0), np.int32), [[]])
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 17
        vs.denoise_batch(src, [[0] * 17], [[t] * 17])
    with pytest.raises(vs.VsError, match="error -1"):               # a source index >= n_src
        vs.denoise_batch(src, [[0, 3]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # candidate 0 is the frame itself: it cannot be missing
        vs.denoise_batch(src, [[-1, 1]], [[t, t]])
    # a negative index ends the list: what lies behind it is not read, not even to be checked
    assert np.array_equal(vs.denoise_batch(src, [[0, -1, 99]], [[t, t, t]]), src[:1])
    with pytest.raises(vs.VsError, match="error -1"):               # a gray format
        vs.denoise_batch(src, [[0, 1]], [[t, t]], fmt=vs.FMT_GRAY8)
    s = vs.Stabilizer(device=0, lag=6)
    assert s.get_denoise() == 0
    for strength, ok in ((0, False), (1, True), (255, True), (256, False)):
        p = vs.denoise_params(strength=strength)
        if ok:
            s.set_denoise(2, p)
            assert vs.denoise_batch(src, [[0, 1]], [[t, t]], params=p).shape == (1, 32, 48, 3)
        else:
            with pytest.raises(vs.VsError, match="error -1"):
                s.set_denoise(3, p)
            with pytest.raises(vs.VsError, match="error -1"):
                vs.denoise_batch(src, [[0, 1]], [[t, t]], params=p)
        assert s.get_denoise() == 2 or strength == 0
    with pytest.raises(vs.VsError, match="error -1"):               # ahead > lag
        s.set_denoise(7)
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_denoise(-1)
    s.set_denoise(6)
    assert s.get_denoise() == 6
    s.set_denoise(0)
    assert s.get_denoise() == 0
    assert vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2, denoise=3).get_denoise() == 3        # every warp mode


_clips = {}


def _clip(bits=8):
    """24 frames with rotation jitter and noise of 3 levels, and three frames in the middle that jump 50 px sideways and back: the alignment
    fails going in and coming out"""
    if bits not in _clips:
        from video_stabilizer_amd import synth
        a = R.noisy_clip(synth, W, H, 21, 11, 3.0, bits=bits, jitter_b=0.03)[0]
        _clips[bits] = np.concatenate([a[:10], np.roll(a[10:13], 50, axis=2), a[10:]])
    return _clips[bits]


def test_denoise_leaves_transforms_state_and_has_output_alone(gpu_vs):
    vs = gpu_vs
    frames = _clip()
    kw = dict(device=0, lag=5, crop_pixels=8, select_mode=vs.SELECT_DEVICE)
    s_on, s_off = [], []
    on = frame_by_frame(vs.Stabilizer(denoise=4, **kw), frames, s_on)
    off = frame_by_frame(vs.Stabilizer(**kw), frames, s_off)
    assert s_on == s_off
    assert not all(s[2] for s in s_off[1:]), "the jump no longer makes the alignment fail: the test input has to change"
    assert sorted(on) == sorted(off) and any(not np.array_equal(on[k], off[k]) for k in on)


def test_denoise_off_is_the_plain_stabilizer_and_a_reset_ends_the_list(gpu_vs):
    """off by default; off after on is a handle that never had it; on in mid-sequence takes effect with the next output frame and equals a
    handle that had it from the start.  After a reset nothing that came before is a candidate: the frames equal a fresh handle's"""
    vs = gpu_vs
    frames = _clip()
    kw = dict(device=0, lag=5, crop_pixels=0)
    a, b, c = vs.Stabilizer(**kw), vs.Stabilizer(**kw), vs.Stabilizer(denoise=3, **kw)
    changed = False
    for i, f in enumerate(frames):
        if i == 7:
            a.set_denoise(3)
        if i == 16:
            a.set_denoise(0)
        oa, ob, oc = a.process(f), b.process(f), c.process(f)
        assert (oa is None) == (ob is None) == (oc is None)
        if oa is None:
            continue
        if 7 <= i < 16:
            assert np.array_equal(oa, oc), i
            changed |= not np.array_equal(oa, ob)
        else:
            assert np.array_equal(oa, ob), i
    assert changed
    st = vs.Stabilizer(denoise=4, **kw)
    for f in frames[:9]:
        st.process(f)
    st.reset()
    got = frame_by_frame(st, frames[9:])
    want = frame_by_frame(vs.Stabilizer(denoise=4, **kw), frames[9:])
    assert sorted(got) == sorted(want) and len(want) > 3 and all(np.array_equal(got[k], want[k]) for k in want)


def _kernel_level(vs, frames, fmt, ahead, deblur, fill, kw):
    """the engine's outputs rebuilt from the kernel-level calls: measurements from a capi.Aligner on the same frames, corrections from a plain
    stabilizer's state, candidates composed here with the host algebra; deblur, denoise, warp, fill"""
    n, h, w, _ = frames.shape
    lag, crop = kw["lag"], kw["crop_pixels"]
    mode = kw.get("warp_mode", vs.WARP_BILINEAR_CV)
    maxv = 255 if frames.dtype == np.uint8 else 1023
    status, meas = vs.Aligner(device=0, select_mode=vs.SELECT_DEVICE).align_batch(frames, fmt=fmt)
    st = vs.Stabilizer(device=0, select_mode=vs.SELECT_DEVICE, **kw)
    due = {}
    for i, f in enumerate(frames):
        if st.process(f) is not None:
            due[i - lag] = vs.Transform.of(*st.state()[1].tup())
        assert st.state()[0].tup() == meas[i].tup() and st.state()[2] == bool(status[i])
    ks = sorted(due)
    ended_early = 0
    targets = frames[ks]
    if deblur:
        S = vs.sharpness_batch(frames, fmt=fmt)
        lists = [EM.lookahead_candidates(vs, k, deblur, meas, status) for k in ks]
        targets = vs.bgr_deblur_batch(frames, S, [l[0] for l in lists], [l[1] for l in lists], fmt=fmt)
    roi = (crop, crop, w - 2 * crop, h - 2 * crop)
    outs = {}
    for i, k in enumerate(ks):
        cf, ct = EM.lookahead_candidates(vs, k, ahead, meas, status)
        ended_early += cf[-1] < 0
        stack = np.concatenate([targets[i][None], frames])          # (frame 0 of the stack: the target; frame j + 1: input frame j)
        clean = vs.denoise_batch(stack, [[0] + [f + 1 if f >= 0 else -1 for f in cf[1:]]], [ct], fmt=fmt)[0]
        Ck = vs.t_inverse(due[k])
        if fill:
            ff, ft = EM.fill_candidates(vs, k, fill, meas, status, Ck)
            ff = [0] + [j + 1 for j in ff[1:]] + [-1] * (fill + 1 - len(ff))
            ft += [vs.Transform.of()] * (fill + 1 - len(ft))
            stack = np.concatenate([clean[None], frames])
            outs[k] = vs.bgr_image_warp_fill_batch(stack, [ff], [ft], roi=roi, border=kw.get("warp_border", vs.BORDER_CONSTANT), max_value=maxv)[0]
        else:
            t = Ck if mode == vs.WARP_BILINEAR_CV else vs.t_inverse(Ck)
            outs[k] = vs.bgr_image_warp_roi_batch(clean[None], [t], roi, mode=mode, border=kw.get("warp_border", vs.BORDER_CONSTANT), max_value=maxv)[0]
    assert ended_early > 0                                           # a failed alignment ended some lists
    return outs


CASES = {"cv": dict(), "cv_fill": dict(border_fill=3), "cv_deblur": dict(deblur=3), "cv_fill_deblur": dict(border_fill=3, deblur=3),
         "lanczos2": dict(warp_mode=0), "cv_10bit": dict()}


def _case_kw(case):
    kw = dict(lag=5, crop_pixels=0 if "fill" in case else 8)
    kw.update(CASES[case])
    return kw


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_route_equals_the_kernel_level_calls(gpu_vs, case):
    """process frame by frame == process_batch (one call; split calls) == device memory == the kernel-level calls, with and without the fill,
    with and without deblur, once with a Lanczos2 warp; a scene cut in the middle"""
    vs = gpu_vs
    bits = 10 if case == "cv_10bit" else 8
    frames = _clip(bits)
    n = len(frames)
    fmt = vs.FMT_BGR8 if bits == 8 else vs.FMT_BGR10
    kw = _case_kw(case)
    want = _kernel_level(vs, frames, fmt, 4, kw.get("deblur", 0), kw.get("border_fill", 0),
                         {k: v for k, v in kw.items() if k not in ("deblur", "border_fill")})
    kw = dict(device=0, select_mode=vs.SELECT_DEVICE, denoise=4, **kw)
    ref = frame_by_frame(vs.Stabilizer(**kw), frames)
    assert sorted(ref) == sorted(want)
    for k in want:
        assert np.array_equal(ref[k], want[k]), (k, int((ref[k] != want[k]).sum()))
    off = frame_by_frame(vs.Stabilizer(**dict(kw, denoise=0)), frames)
    assert sum(int((ref[k] != off[k]).sum()) for k in ref) > 0.2 * sum(ref[k].size for k in ref)      # the pass did something
    assert_every_route_equals(vs, kw, frames, ref, (3, 1, 9, 2, n - 15))


@pytest.mark.parametrize("case", ["cv", "cv_fill_deblur"])
def test_engine_equals_the_engine_model(gpu_vs, oracle, case):
    vs, O = gpu_vs, oracle
    frames = _clip()
    kw = _case_kw(case)
    fill, deblur = kw.pop("border_fill", 0), kw.pop("deblur", 0)
    cvinv = lambda t, w, h: vs.cv_inverse_matrix(vs.Transform.of(*t.tup()), w, h)
    model = EM.engine_model(O, frames, cvinv=cvinv, deblur=deblur, denoise=4, fill=fill, **kw).outs
    got = frame_by_frame(vs.Stabilizer(device=0, denoise=4, deblur=deblur, border_fill=fill, **kw), frames)
    plain = frame_by_frame(vs.Stabilizer(device=0, deblur=deblur, border_fill=fill, **kw), frames)
    assert sorted(got) == sorted(model)
    diff = sum(int((got[k] != model[k]).sum()) for k in model)
    total = sum(model[k].size for k in model)
    moved = sum(int((got[k] != plain[k]).sum()) for k in model)
    print("%s: %d of %d samples differ from the engine model (share %.3g); the pass changed %d samples" % (case, diff, total, diff / total, moved))
    assert moved > 0.2 * total
    assert diff <= 1e-4 * total


@pytest.mark.parametrize("extra", [dict(), dict(deblur=3, border_fill=2)], ids=["denoise", "deblur_denoise_fill"])
def test_chunked_and_pipelined_batches(gpu_vs, monkeypatch, extra):
    """a device-resident clip long enough for the time chunks (denoise and warps on their own stream, the next chunk's alignment prefetched) and
    a host batch long enough for the upload / compute / download pipeline, against process_batch calls that stay below both thresholds"""
    import torch
    vs = gpu_vs
    w, h, n = 320, 240, 260
    frames = _plain_clip(n, 9, w=w, h=h, pan=0.2)
    monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(37 * w * h * 3))  # host batches: upload chunks of 37 frames (read at every call)
    kw = dict(device=0, lag=6, crop_pixels=0, denoise=4, **extra)
    st = vs.Stabilizer(**kw)
    ref = np.zeros_like(frames)
    ref_has = []
    for p in range(0, n, 20):                                        # short calls: one chunk each, no overlap
        o, hs = st.process_batch(frames[p:p + 20])
        ref[p:p + 20] = o
        ref_has += hs
    plain, _ = vs.Stabilizer(**dict(kw, denoise=0)).process_batch(frames[:40])
    assert not np.array_equal(plain, ref[:40])
    out, has = vs.Stabilizer(**kw).process_batch(frames)            # host memory, one call
    assert has == ref_has and np.array_equal(out, ref)
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    st = vs.Stabilizer(**kw)
    for _ in range(2):                                               # (the second call reuses the scratch)
        st.reset()
        dout.zero_()
        r, hs = st.process_batch_device(dev.data_ptr(), n, w, h, vs.FMT_BGR8, dout.data_ptr())
        torch.cuda.synchronize()
        assert hs == ref_has and np.array_equal(dout.cpu().numpy(), ref)


CLIP_CASES = {"plain": dict(), "fill": dict(border_fill=3, crop_pixels=0), "deblur": dict(deblur=3), "fill_deblur": dict(border_fill=3, crop_pixels=0, deblur=3)}


@pytest.mark.parametrize("case", sorted(CLIP_CASES))
def test_process_clips_and_size_change(gpu_vs, case):
    """process_clips on host and device memory (the clip groups: deblur, denoise, warps and fill on the warp stream, the scratch areas shared by
    the groups) against one frame-by-frame handle per clip, with and without the fill, with and without deblur"""
    import torch
    vs = gpu_vs
    n_clips, fpc = 4, 34
    clips = [_plain_clip(fpc, 20 + c) for c in range(n_clips)]
    kw = dict(dict(device=0, lag=5, crop_pixels=8, denoise=4), **CLIP_CASES[case])
    crop = kw["crop_pixels"]
    ref = [frame_by_frame(vs.Stabilizer(**kw), c) for c in clips]
    allf = np.concatenate(clips)
    out, has = vs.Stabilizer(**kw).process_clips(allf, n_clips)
    dev = torch.from_numpy(allf).cuda()
    dout = torch.zeros((n_clips * fpc, H - 2 * crop, W - 2 * crop, 3), dtype=torch.uint8, device="cuda")
    r, dhas = vs.Stabilizer(**kw).process_clips_device(dev.data_ptr(), n_clips, fpc, W, H, vs.FMT_BGR8, dout.data_ptr())
    torch.cuda.synchronize()
    dres = dout.cpu().numpy()
    assert has == dhas
    off = frame_by_frame(vs.Stabilizer(**dict(kw, denoise=0)), clips[0])
    assert any(not np.array_equal(off[k], ref[0][k]) for k in off)   # the pass does something on these clips
    for c in range(n_clips):
        for i in range(fpc):
            assert bool(has[c * fpc + i]) == (i - 5 in ref[c])
            if has[c * fpc + i]:                                     # no frame of the next clip is ever a candidate
                assert np.array_equal(out[c * fpc + i], ref[c][i - 5]), (c, i)
                assert np.array_equal(dres[c * fpc + i], ref[c][i - 5]), (c, i)
    # a size change starts a new clip: the frames of the old size are no candidates
    small = _plain_clip(14, 31, w=256, h=192)
    st = vs.Stabilizer(**kw)
    for f in clips[0][:9]:
        st.process(f)
    got = frame_by_frame(st, small)
    want = frame_by_frame(vs.Stabilizer(**kw), small)
    assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("throwing", [False, True])
def test_denoised_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    """every allocation of a denoised, deblurred, filled process_batch failed once, both signs; the handle recovers.  A handle whose denoise
    was switched on and off again makes the allocations of one that never had it -- the deblurred, filled call of tests/test_deblur_gpu.py --
    and denoise on makes exactly one more: the scratch frames."""
    vs = gpu_vs
    frames = _plain_clip(16, 7)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    kw = dict(device=0, lag=4, smoother_memory=2, crop_pixels=8, deblur=3, border_fill=2)

    def off_again():
        s = vs.Stabilizer(denoise=3, **kw)
        s.set_denoise(0)
        return s
    plain = walk(vs, lambda: vs.Stabilizer(device=0, lag=4, smoother_memory=2, crop_pixels=8), call, 1, throwing)
    never = walk(vs, lambda: vs.Stabilizer(**kw), call, plain + 2, throwing)
    off = walk(vs, off_again, call, plain + 2, throwing)
    on = walk(vs, lambda: vs.Stabilizer(denoise=3, **kw), call, plain + 3, throwing)
    print("denoised process_batch: %d allocations failed one by one (%s); %d with denoise off, %d plain" % (on, "throwing" if throwing else "error code", off, plain))
    assert off == never
    assert on == off + 1
    assert (plain, off, on) == (20, 22, 23)                          # as measured when this was written


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
from video_stabilizer_amd import capi as G, synth
dig = hashlib.sha256()
def put(*xs):
    for x in xs:
        dig.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
rng = np.random.default_rng(77)
w, h, n_src = 203, 149, 5
for dtype, maxv, fmt in ((np.uint8, 255, G.FMT_BGR8), (np.uint16, 1023, G.FMT_BGR10)):
    base = rng.integers(0, maxv + 1, (h, w, 3))
    src = np.clip(base[None] + rng.integers(-6, 7, (n_src, h, w, 3)) * ((maxv + 1) // 256), 0, maxv).astype(dtype)
    cf = np.array([[4, 0, -1, -1], [1, -1, -1, -1], [2, 3, 4, 0], [3, 4, -1, 2], [0, 1, 2, 3]], np.int32)
    ct = [[G.Transform.of(rng.uniform(-0.002, 0.002), rng.uniform(-0.003, 0.003), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)) for _ in range(4)] for _ in range(5)]
    ct[0] = [G.Transform.of(0.0, 0.0, 5000.0 + 100 * c, -3000.0) for c in range(4)]          # output 0: every map leaves the frame
    put(G.denoise_batch(src, cf, ct, fmt=fmt))
    put(G.denoise_batch(src, cf, ct, fmt=fmt, src_stride=3 * w + 7, dst_stride=3 * w + 5))
clip = synth.make_clip(320, 240, 20, seed=5, channels=3)[0]
clip = np.concatenate([clip[:9], synth.make_clip(320, 240, 3, seed=77, channels=3)[0], clip[9:]])
for kw in (dict(denoise=4), dict(denoise=4, deblur=3, border_fill=3, crop_pixels=0), dict(denoise=2, warp_mode=G.WARP_LANCZOS2)):
    kw = dict(dict(device=0, lag=5, crop_pixels=8), **kw)
    s = G.Stabilizer(**kw)
    for fr in clip:
        o = s.process(fr)
        put(o is None)
        if o is not None:
            put(o)
    out, has = G.Stabilizer(**kw).process_batch(clip)
    put(has, out[np.array(has, bool)])
print("DIGEST", dig.hexdigest())
"""

_digests = {}


def _digest(byte):
    if byte not in _digests:
        env = dict(os.environ)
        env.pop("VS_TEST_POISON_ALLOC", None)
        if byte is not None:
            env["VS_TEST_POISON_ALLOC"] = str(byte)
            env["VS_TEST_HOOKS"] = "1"
        out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        _digests[byte] = [line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1]
    return _digests[byte]


@pytest.mark.parametrize("byte", [255, None], ids=["0xff", "unpoisoned"])
def test_denoise_does_not_depend_on_what_fresh_allocations_contain(gpu_vs, byte):
    # one child process per fill byte; every case compares with the zero-filled run (the first case pays for both)
    assert _digest(byte) == _digest(0)


def test_video_test_denoise_writes_what_the_library_returns(gpu_vs, tmp_path):
    frames = _clip()
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("noisy_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    exe = os.path.join(ROOT, "apps", "bin", "vs_video_test")
    r = subprocess.run([exe, str(d), str(tmp_path / "out"), "--crop", "0", "--denoise", "4", "--denoise-strength", "16", "--chunk", "13"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = gpu_vs.Stabilizer(device=0, crop_pixels=0, denoise=4, denoise_params=gpu_vs.denoise_params(strength=16))
    want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_" + raw.name), np.uint8).reshape(-1, H, W, 3)
    assert np.array_equal(got, want)
    st24 = gpu_vs.Stabilizer(device=0, crop_pixels=0, denoise=4)
    assert not np.array_equal(want, np.stack([o for o in (st24.process(f) for f in frames) if o is not None]))
    r = subprocess.run([exe, str(d), str(tmp_path / "out2"), "--denoise", "4", "--denoise-strength", "256"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "vs_stabilizer_set_denoise" in r.stderr
