"""Deblur by transfer on the GPU (include/vs_amd.h: vs_bgr_sharpness_batch, vs_bgr_deblur_batch, vs_stabilizer_set_deblur) against the rule's
restatement (tests/_deblur_ref.py).  Kernel level: np.array_equal -- the rule fixes every rounding.  Engine against the kernel-level calls fed
with candidates built here from a capi.Aligner's measurements: np.array_equal (the same host algebra, the same doubles).  Engine against the
engine model on the CPU oracle's transforms: the two engines' transforms agree to about 1e-12 but not bit for bit and a nearest-sample decision
can flip on that, so the gate there is DESIGN section 14's share -- at most 1e-4 of the samples differ.  Engine routes against each other:
np.array_equal."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _deblur_ref as R
import _engine_model as EM
from _stab_routes import assert_every_route_equals, frame_by_frame, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240
FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}


def _cvinv(vs):
    return lambda t, w, h: vs.cv_inverse_matrix(vs.Transform.of(*t.tup()), w, h)


def _content(rng, kind, n, w, h, dtype, maxv):
    if kind == "noise":
        return rng.integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)
    if kind == "constant":
        return np.full((n, h, w, 3), maxv, dtype)
    yy, xx = np.mgrid[0:h, 0:w]
    period = 1 if kind == "checker1" else 2
    return np.broadcast_to(((((xx // period + yy // period) & 1) * maxv)[None, :, :, None]), (n, h, w, 3)).astype(dtype)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_sharpness_equals_the_rule(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    # (widths that are multiples of 4 take the dword-load kernel when the rows are aligned, the others the per-sample one)
    shapes = [(3, 3), (4, 7), (7, 3), (4, 3), (8, 5), (63, 40), (64, 33), (65, 35), (125, 131), (203, 149), (252, 40), (256, 37), (260, 34), (512, 70)]
    shapes += [(1920, 1080)] if fmt in ("bgr8", "bgr10") else []
    for w, h in shapes:
        for kind in ("noise", "constant", "checker1", "checker2") if w < 1000 else ("noise",):
            src = _content(rng, kind, 3 if w < 1000 else 2, w, h, dtype, maxv)
            src[-1] //= 3
            want = R.sharpness_batch(src, bits)
            got = vs.sharpness_batch(src, fmt=code)
            assert np.array_equal(got, want), (w, h, kind, got, want)
            if w < 1000:
                assert np.array_equal(vs.sharpness_batch(src, fmt=code, src_stride=3 * w + 7), want), (w, h, kind, "pitched")
                assert np.array_equal(vs.sharpness_batch(src, fmt=code, src_stride=3 * w + 8), want), (w, h, kind, "pitched, aligned")
    # frames too small to have an interior
    assert list(vs.sharpness_batch(np.full((2, 2, 9, 3), maxv, dtype), fmt=code)) == [0, 0]
    assert list(vs.sharpness_batch(np.full((1, 5, 1, 3), maxv, dtype), fmt=code)) == [0]


def _graded(rng, n, w, h, dtype, maxv):
    """frames of one scene at different contrasts, so that their sharpness differs by large factors; frame 1 is black (S = 0), frames 2 and 3
    are identical (a tie), the last frame is the sharpest"""
    base = rng.integers(0, maxv + 1, (h // 4 + 2, w // 4 + 2, 3))
    up = np.repeat(np.repeat(base, 4, 0), 4, 1)[:h, :w]
    out = []
    for i in range(n):
        k = (i + 1) / n
        f = np.clip(up * k + maxv * (1 - k) / 2 + rng.integers(-2, 3, up.shape), 0, maxv)
        out.append(f)
    out = np.stack(out).astype(dtype)
    out[1] = 0
    out[3] = out[2]
    return out


def _cand_lists(vs, rng, n_out, n_cand, n_src, w, h):
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    cf[0, 0] = 1                                                     # S_k = 0
    cf[1, 0] = 2                                                     # a tie among the candidates
    if n_cand > 1:
        cf[1, 1] = 3
    cf[2, 0] = n_src - 1                                             # the sharpest frame: a copy
    ct = []
    for o in range(n_out):
        row = [vs.Transform.of(*rng.uniform(-1, 1, 4))]               # (candidate 0's transform is ignored)
        for c in range(1, n_cand):
            row.append(vs.Transform.of(rng.uniform(-0.04, 0.04), rng.uniform(-0.05, 0.05), rng.uniform(-0.15, 0.15) * w, rng.uniform(-0.15, 0.15) * h))
        if n_cand >= 3:
            row[2] = vs.Transform.of(0.0, 0.0, 3.0 * w, -2.0 * h)     # a map that leaves the frame altogether
        if n_cand >= 4 and o % 2 == 1:
            cf[o, 3] = -1                                            # the list ends early
        ct.append(row)
    return cf, ct


@pytest.mark.parametrize("shape", [(203, 149), (260, 75)], ids=["203x149", "260x75"])     # (the per-sample kernel; four pixels per lane)
@pytest.mark.parametrize("n_cand", [1, 4, 16])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10", "bgr12", "bgr16"])
def test_deblur_batch_equals_the_rule(gpu_vs, fmt, n_cand, shape):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(1000 * bits + n_cand)
    (w, h), n_src, n_out = shape, 7, 6
    src = _graded(rng, n_src, w, h, dtype, maxv)
    S = vs.sharpness_batch(src, fmt=code)
    assert np.array_equal(S, R.sharpness_batch(src, bits)) and S[1] == 0 and S[2] == S[3] and S[-1] == S.max()
    cf, ct = _cand_lists(vs, rng, n_out, n_cand, n_src, w, h)
    want = R.deblur_batch(_cvinv(vs), src, S, cf, ct, bits, maxv)
    got = vs.bgr_deblur_batch(src, S, cf, ct, fmt=code)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got[2], src[-1])                          # no sharper candidate
    if n_cand > 1:
        assert not np.array_equal(got[0], src[1]) and (got != src[cf[:, 0]]).mean() > 0.05      # the test has teeth
    # pitched rows on both sides, the destination inside a guard band that must stay untouched
    guard = 0x5A if bits == 8 else 0x5A5A
    res, padded = vs.bgr_deblur_batch(src, S, cf, ct, fmt=code, src_stride=3 * w + 7, dst_stride=3 * w + 5, guard=guard)
    assert np.array_equal(res, want)
    assert (padded[:, :, 3 * w:] == guard).all()
    res, padded = vs.bgr_deblur_batch(src, S, cf, ct, fmt=code, src_stride=3 * w + 8, dst_stride=3 * w + 4, guard=guard)     # rows that start on dwords
    assert np.array_equal(res, want)
    assert (padded[:, :, 3 * w:] == guard).all()
    # other parameters
    p = vs.deblur_params(sensitivity=0.5, max_ratio=1.75)
    assert np.array_equal(vs.bgr_deblur_batch(src, S, cf, ct, params=p, fmt=code), R.deblur_batch(_cvinv(vs), src, S, cf, ct, bits, maxv, 0.5, 1.75))


def test_device_memory_equals_host_memory(gpu_vs):
    import torch
    vs = gpu_vs
    rng = np.random.default_rng(5)
    w, h, n_src, n_out, n_cand = 331, 200, 6, 40, 5                  # (40 outputs x 5 candidates: more than a kernel-argument block carries)
    src = _graded(rng, n_src, w, h, np.uint8, 255)
    cf, ct = _cand_lists(vs, rng, n_out, n_cand, n_src, w, h)
    S = vs.sharpness_batch(src)
    want = vs.bgr_deblur_batch(src, S, cf, ct)
    assert np.array_equal(want, R.deblur_batch(_cvinv(vs), src, S, cf, ct, 8, 255))
    dsrc = torch.from_numpy(src).cuda()
    dS = torch.zeros(n_src, dtype=torch.int64, device="cuda")
    dout = torch.zeros((n_out, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vs.sharpness_batch_device(dsrc.data_ptr(), n_src, w, h, vs.FMT_BGR8, dS.data_ptr())
    vs.bgr_deblur_batch_device(dsrc.data_ptr(), n_src, w, h, vs.FMT_BGR8, dS.data_ptr(), cf, ct, dout.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dS.cpu().numpy().view(np.uint64), S)
    assert np.array_equal(dout.cpu().numpy(), want)


def test_argument_errors(gpu_vs):
    vs = gpu_vs
    src = np.zeros((3, 32, 48, 3), np.uint8)
    S = np.zeros(3, np.uint64)
    t = vs.Transform.of(0, 0, 3, 2)
    assert vs.bgr_deblur_batch(src, S, [[0, 1]], [[t, t]]).shape == (1, 32, 48, 3)
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 0
        vs.bgr_deblur_batch(src, S, np.zeros((1, 0), np.int32), [[]])
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 17
        vs.bgr_deblur_batch(src, S, [[0] * 17], [[t] * 17])
    with pytest.raises(vs.VsError, match="error -1"):               # a source index >= n_src
        vs.bgr_deblur_batch(src, S, [[0, 3]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # candidate 0 is the frame itself: it cannot be missing
        vs.bgr_deblur_batch(src, S, [[-1, 1]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # a gray format
        vs.bgr_deblur_batch(src, S, [[0, 1]], [[t, t]], fmt=vs.FMT_GRAY8)
    with pytest.raises(vs.VsError, match="error -1"):
        vs.sharpness_batch(src, fmt=7)
    with pytest.raises(vs.VsError, match="error -1"):
        vs.bgr_deblur_batch(src, S, [[0, 1]], [[t, t]], params=vs.deblur_params(sensitivity=0.0))
    s = vs.Stabilizer(device=0, lag=6)
    with pytest.raises(vs.VsError, match="error -1"):               # ahead > lag
        s.set_deblur(7)
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_deblur(-1)
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_deblur(2, vs.deblur_params(max_ratio=-1.0))
    assert s.deblur() == 0
    s.set_deblur(6)
    assert s.deblur() == 6
    s.set_deblur(0)
    assert s.deblur() == 0
    assert vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2, deblur=3).deblur() == 3          # every warp mode


_clips = {}


def _clip(bits=8):
    """40 frames with rotation jitter (a flipped nearest-sample decision then moves single pixels, not a frame), 1 LSB noise, three frames
    motion-blurred along 6 px, and three frames in the middle that jump 50 px sideways and back: the alignment fails going in and coming out"""
    if bits not in _clips:
        from video_stabilizer_amd import synth
        a = R.blurred_clip(synth, W, H, 37, 11, (8, 21, 30), bits=bits, jitter_b=0.03)[0]
        _clips[bits] = np.concatenate([a[:16], np.roll(a[16:19], 50, axis=2), a[16:]])
    return _clips[bits]


def _plain_clip(n, seed, w=W, h=H, **kw):
    from video_stabilizer_amd import synth
    return synth.make_clip(w, h, n, seed=seed, channels=3, **kw)[0]


def test_deblur_leaves_transforms_state_and_has_output_alone(gpu_vs):
    vs = gpu_vs
    frames = _clip()
    kw = dict(device=0, lag=6, crop_pixels=8, select_mode=vs.SELECT_DEVICE)
    s_on, s_off = [], []
    on = frame_by_frame(vs.Stabilizer(deblur=4, **kw), frames, s_on)
    off = frame_by_frame(vs.Stabilizer(**kw), frames, s_off)
    assert s_on == s_off
    assert not all(s[2] for s in s_off[1:]), "the jump no longer makes the alignment fail: the test input has to change"
    assert sorted(on) == sorted(off) and any(not np.array_equal(on[k], off[k]) for k in on)


def test_deblur_off_is_the_plain_stabilizer(gpu_vs):
    """off by default; off after on is a handle that never had it; on in mid-sequence takes effect with the next output frame (the queued
    frames' sharpness is made up then) and equals a handle that had it from the start"""
    vs = gpu_vs
    frames = _clip()
    kw = dict(device=0, lag=6, crop_pixels=0)
    a, b, c = vs.Stabilizer(**kw), vs.Stabilizer(**kw), vs.Stabilizer(deblur=3, **kw)
    assert b.deblur() == 0
    changed = False
    for i, f in enumerate(frames):
        if i == 10:
            a.set_deblur(3)
        if i == 25:
            a.set_deblur(0)
        oa, ob, oc = a.process(f), b.process(f), c.process(f)
        assert (oa is None) == (ob is None) == (oc is None)
        if oa is None:
            continue
        if 10 <= i < 25:
            assert np.array_equal(oa, oc), i
            changed |= not np.array_equal(oa, ob)
        else:
            assert np.array_equal(oa, ob), i
    assert changed


def _kernel_level(vs, frames, fmt, ahead, fill, kw):
    """the engine's outputs rebuilt from the kernel-level calls: measurements from a capi.Aligner on the same frames, corrections from a plain
    stabilizer's state, candidates composed here with the host algebra"""
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
    S = vs.sharpness_batch(frames, fmt=fmt)
    ks = sorted(due)
    cf, ct = [], []
    for k in ks:
        f, t = EM.lookahead_candidates(vs, k, ahead, meas, status)
        cf.append(f)
        ct.append(t)
    sharpened = vs.bgr_deblur_batch(frames, S, cf, ct, fmt=fmt)
    roi = (crop, crop, w - 2 * crop, h - 2 * crop)
    outs = {}
    for i, k in enumerate(ks):
        Ck = vs.t_inverse(due[k])
        if fill:
            ff, ft = EM.fill_candidates(vs, k, fill, meas, status, Ck)
            ff = [0] + [j + 1 for j in ff[1:]] + [-1] * (fill + 1 - len(ff))
            ft += [vs.Transform.of()] * (fill + 1 - len(ft))
            stack = np.concatenate([sharpened[i][None], frames])
            outs[k] = vs.bgr_image_warp_fill_batch(stack, [ff], [ft], roi=roi, border=kw.get("warp_border", vs.BORDER_CONSTANT), max_value=maxv)[0]
        else:
            t = Ck if mode == vs.WARP_BILINEAR_CV else vs.t_inverse(Ck)
            outs[k] = vs.bgr_image_warp_roi_batch(sharpened[i][None], [t], roi, mode=mode, border=kw.get("warp_border", vs.BORDER_CONSTANT), max_value=maxv)[0]
    return outs


@pytest.mark.parametrize("case", ["cv", "cv_fill", "lanczos2", "cv_10bit"])
def test_engine_equals_the_kernel_level_calls(gpu_vs, case):
    vs = gpu_vs
    bits = 10 if case == "cv_10bit" else 8
    frames = _clip(bits)
    fmt = vs.FMT_BGR8 if bits == 8 else vs.FMT_BGR10
    kw = dict(lag=6, crop_pixels=0 if case == "cv_fill" else 8)
    if case == "lanczos2":
        kw["warp_mode"] = vs.WARP_LANCZOS2
    fill = 3 if case == "cv_fill" else 0
    want = _kernel_level(vs, frames, fmt, 4, fill, kw)
    got = frame_by_frame(vs.Stabilizer(device=0, select_mode=vs.SELECT_DEVICE, deblur=4, border_fill=fill, **kw), frames)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("case", ["cv", "cv_fill"])
def test_engine_equals_the_engine_model(gpu_vs, oracle, case):
    vs, O = gpu_vs, oracle
    frames = _clip()
    fill = 3 if case == "cv_fill" else 0
    kw = dict(lag=6, crop_pixels=0 if fill else 8)
    model = EM.engine_model(O, frames, cvinv=_cvinv(vs), deblur=4, fill=fill, **kw).outs
    got = frame_by_frame(vs.Stabilizer(device=0, deblur=4, border_fill=fill, **kw), frames)
    plain = frame_by_frame(vs.Stabilizer(device=0, **kw), frames)
    assert sorted(got) == sorted(model)
    diff = sum(int((got[k] != model[k]).sum()) for k in model)
    total = sum(model[k].size for k in model)
    moved = sum(int((got[k] != plain[k]).sum()) for k in model)
    print("%s: %d of %d samples differ from the engine model (share %.3g); the pass changed %d samples" % (case, diff, total, diff / total, moved))
    assert moved > 0.05 * total
    assert diff <= 1e-4 * total


@pytest.mark.parametrize("case", ["cv", "cv_fill", "lanczos2_sep", "cv_10bit"])
def test_every_route_gives_the_same_frames(gpu_vs, case):
    """process frame by frame == process_batch (one call; split calls) == device memory, with deblur on; a scene cut in the middle"""
    vs = gpu_vs
    bits = 10 if case == "cv_10bit" else 8
    frames = _clip(bits)
    n = len(frames)
    kw = dict(device=0, lag=6, crop_pixels=8, deblur=4)
    if case == "cv_fill":
        kw["border_fill"] = 3
    if case == "lanczos2_sep":
        kw["warp_mode"] = vs.WARP_LANCZOS2_SEP
    ref = frame_by_frame(vs.Stabilizer(**kw), frames)
    assert_every_route_equals(vs, kw, frames, ref, (3, 1, 9, 2, 11, n - 26))


@pytest.mark.parametrize("fill", [0, 3])
def test_chunked_and_pipelined_batches(gpu_vs, monkeypatch, fill):
    """a device-resident clip long enough for the time chunks (deblur and warps on their own stream, the next chunk's alignment prefetched) and
    a host batch long enough for the upload / compute / download pipeline, against process_batch calls that stay below both thresholds"""
    import torch
    vs = gpu_vs
    w, h, n = 320, 240, 260
    frames = _plain_clip(n, 9, w=w, h=h, pan=0.2)
    monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(37 * w * h * 3))  # host batches: upload chunks of 37 frames (read at every call)
    kw = dict(device=0, lag=6, crop_pixels=0, deblur=4, border_fill=fill)
    st = vs.Stabilizer(**kw)
    ref = np.zeros_like(frames)
    ref_has = []
    for p in range(0, n, 20):                                        # short calls: one chunk each, no overlap
        o, hs = st.process_batch(frames[p:p + 20])
        ref[p:p + 20] = o
        ref_has += hs
    plain, _ = vs.Stabilizer(device=0, lag=6, crop_pixels=0, border_fill=fill).process_batch(frames[:40])
    assert not np.array_equal(plain, ref[:40])
    out, has = vs.Stabilizer(**kw).process_batch(frames)            # host memory, one call
    assert has == ref_has and np.array_equal(out, ref)
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    st = vs.Stabilizer(**kw)
    for _ in range(2):                                               # (the second call reuses the scratch and the sharpness blocks)
        st.reset()
        dout.zero_()
        r, hs = st.process_batch_device(dev.data_ptr(), n, w, h, vs.FMT_BGR8, dout.data_ptr())
        torch.cuda.synchronize()
        assert hs == ref_has and np.array_equal(dout.cpu().numpy(), ref)


def test_process_clips_and_size_change(gpu_vs):
    import torch
    vs = gpu_vs
    n_clips, fpc = 4, 34
    clips = [_plain_clip(fpc, 20 + c) for c in range(n_clips)]
    kw = dict(device=0, lag=5, crop_pixels=8, deblur=4)
    ref = [frame_by_frame(vs.Stabilizer(**kw), c) for c in clips]
    allf = np.concatenate(clips)
    out, has = vs.Stabilizer(**kw).process_clips(allf, n_clips)
    dev = torch.from_numpy(allf).cuda()
    dout = torch.zeros((n_clips * fpc, H - 16, W - 16, 3), dtype=torch.uint8, device="cuda")
    r, dhas = vs.Stabilizer(**kw).process_clips_device(dev.data_ptr(), n_clips, fpc, W, H, vs.FMT_BGR8, dout.data_ptr())
    torch.cuda.synchronize()
    dres = dout.cpu().numpy()
    assert has == dhas
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
def test_deblurred_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    vs = gpu_vs
    frames = _plain_clip(16, 7)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    plain = walk(vs, lambda: vs.Stabilizer(device=0, lag=4, smoother_memory=2, crop_pixels=8), call, 1, throwing)
    n = walk(vs, lambda: vs.Stabilizer(device=0, lag=4, smoother_memory=2, crop_pixels=8, deblur=3, border_fill=2), call, plain + 2, throwing)
    print("deblurred process_batch: %d allocations failed one by one (%s); %d without deblur" % (n, "throwing" if throwing else "error code", plain))


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
    src = rng.integers(0, maxv + 1, (n_src, h, w, 3)).astype(dtype)
    for i in range(n_src):
        src[i] = src[i] // (i + 1)
    S = G.sharpness_batch(src, fmt=fmt)
    put(S)
    cf = np.array([[4, 0, -1, -1], [1, -1, -1, -1], [2, 3, 4, 0], [3, 4, -1, 2], [0, 1, 2, 3]], np.int32)
    ct = [[G.Transform.of(rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-25, 25), rng.uniform(-18, 18)) for _ in range(4)] for _ in range(5)]
    ct[0] = [G.Transform.of(0.0, 0.0, 5000.0 + 100 * c, -3000.0) for c in range(4)]          # output 0: every map leaves the frame
    put(G.bgr_deblur_batch(src, S, cf, ct, fmt=fmt))
    put(G.bgr_deblur_batch(src, S, cf, ct, fmt=fmt, src_stride=3 * w + 7, dst_stride=3 * w + 5))
clip = synth.make_clip(320, 240, 30, seed=5, channels=3)[0]
clip = np.concatenate([clip[:14], synth.make_clip(320, 240, 3, seed=77, channels=3)[0], clip[14:]])
for kw in (dict(deblur=4), dict(deblur=4, border_fill=3, crop_pixels=0), dict(deblur=2, warp_mode=G.WARP_LANCZOS2)):
    kw = dict(dict(device=0, lag=6, crop_pixels=8), **kw)
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


@pytest.mark.parametrize("byte", [255, 0x7f, None], ids=["0xff", "0x7f", "unpoisoned"])
def test_deblur_does_not_depend_on_what_fresh_allocations_contain(gpu_vs, byte):
    # one child process per fill byte; every case compares with the zero-filled run (the first case pays for both)
    assert _digest(byte) == _digest(0)


def test_video_test_deblur_writes_what_the_library_returns(gpu_vs, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    frames = _clip()
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    r = subprocess.run([os.path.join(ROOT, "apps", "bin", "vs_video_test"), str(d), str(tmp_path / "out"), "--crop", "0", "--deblur", "4", "--chunk", "13"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = gpu_vs.Stabilizer(device=0, crop_pixels=0, deblur=4)
    want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_" + raw.name), np.uint8).reshape(-1, H, W, 3)
    assert np.array_equal(got, want)
    plain = gpu_vs.Stabilizer(device=0, crop_pixels=0)
    assert not np.array_equal(want, np.stack([o for o in (plain.process(f) for f in frames) if o is not None]))
    r = subprocess.run([os.path.join(ROOT, "apps", "bin", "vs_video_test"), str(d), str(tmp_path / "out2"), "--deblur", "40"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "vs_stabilizer_set_deblur" in r.stderr
