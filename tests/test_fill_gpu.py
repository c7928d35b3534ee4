"""Border fill on the GPU (include/vs_amd.h: vs_bgr_image_warp_fill_batch, vs_stabilizer_set_border_fill) against the rule's reference
(tests/_fill_ref.py: numpy on top of the CPU oracle).  Kernel level: np.array_equal.  Engine against the engine model: the transforms of the
two engines agree to about 1e-12 but not bit for bit and a coverage decision can flip on that, so the gate there is SURVEY 8(d)'s share -- at
most 1e-4 of the samples differ (the reference alone moves no sample under a 1e-12 perturbation of every transform and at most 4.4e-7 of them
under 1e-9).  Engine routes against each other: np.array_equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _engine_model as EM
import _fill_ref as R
from _stab_routes import assert_every_route_equals, frame_by_frame, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240


def _gt(vs, t):
    return vs.Transform.of(*t.tup())


def _frames(rng, n, w, h, dtype, maxv):
    # smooth-ish content with noise on top: every rounding of the sampler matters somewhere
    base = rng.integers(0, maxv + 1, (n, h // 8 + 2, w // 8 + 2, 3))
    up = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :h, :w]
    return np.clip(up + rng.integers(-3, 4, up.shape), 0, maxv).astype(dtype)


def _cands(O, rng, n_out, n_cand, n_src, w, h):
    """candidate lists with shifts, rotation and zoom; lists cut short by -1; a candidate named twice"""
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    ct = []
    for o in range(n_out):
        own = (rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-0.12, 0.12) * w, rng.uniform(-0.12, 0.12) * h)
        row = [O.Transform.of(*own)]
        for c in range(1, n_cand):
            row.append(O.Transform.of(own[0] + rng.uniform(-0.03, 0.03), own[1] + rng.uniform(-0.02, 0.02),
                                      own[2] + rng.uniform(-0.1, 0.1) * w, own[3] + rng.uniform(-0.1, 0.1) * h))
        ct.append(row)
        if n_cand >= 3 and o % 2 == 1:
            cf[o, rng.integers(1, n_cand)] = -1                     # the list ends early
        if n_cand >= 3 and o % 2 == 0:
            cf[o, 2], row[2] = cf[o, 1], row[1]                      # the same candidate twice
    return cf, ct


@pytest.mark.parametrize("n_cand", [1, 2, 5, 16])
@pytest.mark.parametrize("bits,maxv", [(8, 255), (10, 1023)])
def test_fill_batch_equals_the_rule(gpu_vs, oracle, bits, maxv, n_cand):
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(100 * bits + n_cand)
    w, h, n_src, n_out = 203, 149, 6, 5
    src = _frames(rng, n_src, w, h, np.uint8 if bits == 8 else np.uint16, maxv)
    cf, ct = _cands(O, rng, n_out, n_cand, n_src, w, h)
    # output 3: the frame itself covers NOTHING (everything comes from the candidates, or is border)
    ct[3][0] = O.Transform.of(0.0, 0.0, 5000.0, -3000.0)
    assert not R.covered(O, ct[3][0], w, h).any()
    gct = [[_gt(vs, t) for t in row] for row in ct]
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        want = R.fill_batch(O, src, cf, ct, border, maxv)
        got = vs.bgr_image_warp_fill_batch(src, cf, gct, border=border, max_value=maxv)
        assert np.array_equal(got, want), (border, int((got != want).sum()))
        # pitched rows on both sides
        got = vs.bgr_image_warp_fill_batch(src, cf, gct, border=border, max_value=maxv, src_stride=3 * w + 7, dst_stride=3 * w + 5)
        assert np.array_equal(got, want)
    # a window that is not tile-aligned == the crop of the full result
    roi = (13, 9, 131, 77)
    got = vs.bgr_image_warp_fill_batch(src, cf, gct, roi=roi, border=vs.BORDER_CONSTANT, max_value=maxv, dst_stride=3 * 131 + 2)
    assert np.array_equal(got, want_roi(O, src, cf, ct, maxv, roi))
    if n_cand > 1:                                                   # the test has teeth: the candidates changed pixels
        plain = R.fill_batch(O, src, cf[:, :1], [r[:1] for r in ct], O.BORDER_CONSTANT, maxv)
        assert (plain != R.fill_batch(O, src, cf, ct, O.BORDER_CONSTANT, maxv)).any()


def want_roi(O, src, cf, ct, maxv, roi):
    x, y, rw, rh = roi
    return R.fill_batch(O, src, cf, ct, O.BORDER_CONSTANT, maxv)[:, y:y + rh, x:x + rw]


@pytest.mark.parametrize("bits,maxv", [(8, 255), (10, 1023)])
def test_one_candidate_is_the_plain_roi_warp(gpu_vs, bits, maxv):
    vs = gpu_vs
    rng = np.random.default_rng(7 + bits)
    w, h, n = 331, 200, 4
    src = _frames(rng, n, w, h, np.uint8 if bits == 8 else np.uint16, maxv)
    ts = [vs.Transform.of(rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-30, 30), rng.uniform(-20, 20)) for _ in range(n)]
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        for roi in ((0, 0, w, h), (32, 32, w - 64, h - 64)):
            a = vs.bgr_image_warp_roi_batch(src, ts, roi, mode=vs.WARP_BILINEAR_CV, border=border, max_value=maxv)
            b = vs.bgr_image_warp_fill_batch(src, np.arange(n, dtype=np.int32)[:, None], [[t] for t in ts], roi=roi, border=border, max_value=maxv)
            assert np.array_equal(a, b)


def test_device_memory_equals_host_memory(gpu_vs, oracle):
    import torch
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(11)
    w, h, n_src, n_out, n_cand = 203, 149, 6, 5, 5
    src = _frames(rng, n_src, w, h, np.uint8, 255)
    cf, ct = _cands(O, rng, n_out, n_cand, n_src, w, h)
    gct = [[_gt(vs, t) for t in row] for row in ct]
    want = vs.bgr_image_warp_fill_batch(src, cf, gct, border=vs.BORDER_CONSTANT)
    dsrc = torch.from_numpy(src).cuda()
    dout = torch.zeros((n_out, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    arr = (vs.Transform * (n_out * n_cand))(*[t for row in gct for t in row])
    idx = np.ascontiguousarray(cf, np.int32)
    vs._check(vs.lib().vs_bgr_image_warp_fill_batch(C.c_void_p(dsrc.data_ptr()), h * w * 3, n_src, w, h, w * 3, 3, 8, n_out, n_cand,
                                                    idx.ctypes.data_as(C.POINTER(C.c_int32)), arr, vs.BORDER_CONSTANT, 255, 0, 0, w, h,
                                                    C.c_void_p(dout.data_ptr()), h * w * 3, w * 3, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), want)
    assert np.array_equal(want, R.fill_batch(O, src, cf, ct, O.BORDER_CONSTANT, 255))


def test_1080p(gpu_vs, oracle):
    from video_stabilizer_amd import synth
    vs, O = gpu_vs, oracle
    frames, _ = synth.make_clip(1920, 1080, 5, seed=21, channels=3, jitter_t=12.0)
    cf = np.array([[0, 1, 2, 3, 4], [2, 3, 4, 0, 1]], np.int32)
    rng = np.random.default_rng(2)
    ct = []
    for o in range(2):
        own = (0.004, -0.006, 23.5 - 50 * o, -17.25 + 30 * o)
        ct.append([O.Transform.of(*own)] + [O.Transform.of(own[0] + rng.uniform(-0.004, 0.004), own[1] + rng.uniform(-0.004, 0.004),
                                                           own[2] + rng.uniform(-25, 25), own[3] + rng.uniform(-25, 25)) for _ in range(4)])
    want = R.fill_batch(O, frames, cf, ct, O.BORDER_CONSTANT)
    got = vs.bgr_image_warp_fill_batch(frames, cf, [[_gt(vs, t) for t in row] for row in ct], border=vs.BORDER_CONSTANT)
    assert np.array_equal(got, want)


def test_argument_errors(gpu_vs):
    vs = gpu_vs
    src = np.zeros((3, 32, 48, 3), np.uint8)
    t = vs.Transform.of(0, 0, 3, 2)
    ok = vs.bgr_image_warp_fill_batch(src, [[0, 1]], [[t, t]])
    assert ok.shape == (1, 32, 48, 3)
    with pytest.raises(vs.VsError, match="error -1"):               # another channel count
        vs.bgr_image_warp_fill_batch(np.zeros((3, 32, 48, 4), np.uint8), [[0, 1]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):
        vs.bgr_image_warp_fill_batch(np.zeros((3, 32, 48, 1), np.uint8), [[0, 1]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 0
        vs.bgr_image_warp_fill_batch(src, np.zeros((1, 0), np.int32), [[]])
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 17
        vs.bgr_image_warp_fill_batch(src, [[0] * 17], [[t] * 17])
    with pytest.raises(vs.VsError, match="error -1"):               # a source index >= n_src
        vs.bgr_image_warp_fill_batch(src, [[0, 3]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # candidate 0 is the frame itself: it cannot be missing
        vs.bgr_image_warp_fill_batch(src, [[-1, 1]], [[t, t]])
    s = vs.Stabilizer(device=0, lag=6)
    with pytest.raises(vs.VsError, match="error -1"):               # ahead > lag
        s.set_border_fill(7)
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_border_fill(-1)
    s.set_border_fill(6)
    assert s.border_fill() == 6
    s.set_border_fill(0)
    assert s.border_fill() == 0
    lz = vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2)
    with pytest.raises(vs.VsError, match="error -3"):               # a Lanczos2 handle
        lz.set_border_fill(2)
    with pytest.raises(vs.VsError, match="error -3"):
        vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2, border_fill=2)
    assert vs.Stabilizer(device=0, border_fill=3).border_fill() == 3


def _clip(n, seed, bits=8, w=W, h=H, **kw):
    from video_stabilizer_amd import synth
    return synth.make_clip(w, h, n, seed=seed, channels=3, bits=bits, **kw)[0]


def _cut_clip(bits):
    """40 frames with a three-frame scene cut in the middle: the alignment fails there (asserted where the model is run)"""
    a = _clip(30, 5, bits)
    return np.concatenate([a[:14], _clip(3, 77, bits), a[14:]])


def test_fill_off_after_on_is_a_handle_that_never_had_it(gpu_vs):
    vs = gpu_vs
    frames = _clip(30, 5)
    a = vs.Stabilizer(device=0, lag=6, crop_pixels=0)
    b = vs.Stabilizer(device=0, lag=6, crop_pixels=0)
    changed = False
    for i, f in enumerate(frames):
        if i == 10:
            a.set_border_fill(4)
        if i == 20:
            a.set_border_fill(0)
        oa, ob = a.process(f), b.process(f)
        assert (oa is None) == (ob is None)
        if oa is None:
            continue
        if 10 <= i < 20:
            changed |= not np.array_equal(oa, ob)
        else:
            assert np.array_equal(oa, ob), i
    assert changed                                                   # the fill did something while it was on


@pytest.mark.parametrize("crop", [0, 32])
@pytest.mark.parametrize("bits", [8, 10])
def test_engine_equals_the_engine_model(gpu_vs, oracle, bits, crop):
    vs, O = gpu_vs, oracle
    frames = _cut_clip(bits)
    kw = dict(lag=6, crop_pixels=crop)
    model = EM.engine_model(O, frames, fill=4, want_masks=True, **kw)
    st = O.Stabilizer(**kw)
    succ = []
    for f in frames:
        st.process(f)
        succ.append(st.state()[2])
    assert not all(succ[1:]), "the scene cut no longer makes the alignment fail: the test input has to change"
    got = frame_by_frame(vs.Stabilizer(device=0, border_fill=4, **kw), frames)
    assert sorted(got) == sorted(model.outs)
    diff = total = filled = 0
    for k, want in model.outs.items():
        cov0, still_open = model.masks[k]
        diff += int((got[k] != want).sum())
        total += want.size
        filled += int((~cov0 & ~still_open).sum())
    print("%d-bit crop %d: %d of %d samples differ (share %.3g), %d pixels filled" % (bits, crop, diff, total, diff / total, filled))
    if crop == 0:
        assert filled > 0
    # (inside a 32-pixel crop this clip's corrections leave nothing uncovered: the case then checks that the fill pass leaves a covered window alone)
    assert diff <= 1e-4 * total


@pytest.mark.parametrize("bits", [8, 10])
def test_every_route_gives_the_same_frames(gpu_vs, bits):
    """process frame by frame == process_batch (one call; split calls) == device memory, with the fill on; a scene cut in the middle"""
    vs = gpu_vs
    frames = _cut_clip(bits)
    n = len(frames)
    kw = dict(device=0, lag=6, crop_pixels=8, border_fill=4)
    ref = frame_by_frame(vs.Stabilizer(**kw), frames)
    plain = frame_by_frame(vs.Stabilizer(device=0, lag=6, crop_pixels=8), frames)
    assert any(not np.array_equal(ref[k], plain[k]) for k in ref)
    assert_every_route_equals(vs, kw, frames, ref, (3, 1, 9, 2, 11, n - 26))


def test_chunked_and_pipelined_batches(gpu_vs, monkeypatch):
    """a device-resident clip long enough for the time chunks (warps on their own stream, the next chunk's alignment prefetched) and a host batch
    long enough for the upload / compute / download pipeline, against process_batch calls that stay below both thresholds"""
    import torch
    vs = gpu_vs
    w, h, n = 480, 360, 260
    frames = _clip(n, 9, w=w, h=h, pan=0.2)
    monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(37 * w * h * 3))  # host batches: upload chunks of 37 frames (read at every call)
    kw = dict(device=0, lag=6, crop_pixels=0, border_fill=4)
    st = vs.Stabilizer(**kw)
    ref = np.zeros_like(frames)
    ref_has = []
    for p in range(0, n, 20):                                        # short calls: one chunk each, no overlap
        o, hs = st.process_batch(frames[p:p + 20])
        ref[p:p + 20] = o
        ref_has += hs
    plain, _ = vs.Stabilizer(device=0, lag=6, crop_pixels=0).process_batch(frames[:40])
    assert not np.array_equal(plain, ref[:40])
    out, has = vs.Stabilizer(**kw).process_batch(frames)            # host memory, one call
    assert has == ref_has and np.array_equal(out, ref)
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    r, hs = vs.Stabilizer(**kw).process_batch_device(dev.data_ptr(), n, w, h, vs.FMT_BGR8, dout.data_ptr())
    torch.cuda.synchronize()
    assert hs == ref_has and np.array_equal(dout.cpu().numpy(), ref)


def test_process_clips_and_size_change(gpu_vs):
    import torch
    vs = gpu_vs
    n_clips, fpc = 4, 34
    clips = [_clip(fpc, 20 + c) for c in range(n_clips)]
    kw = dict(device=0, lag=5, crop_pixels=8, border_fill=4)
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
    small = _clip(14, 31, w=256, h=192)
    st = vs.Stabilizer(**kw)
    for f in clips[0][:9]:
        st.process(f)
    got = frame_by_frame(st, small)
    want = frame_by_frame(vs.Stabilizer(**kw), small)
    assert sorted(got) == sorted(want) and all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("throwing", [False, True])
def test_filled_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    vs = gpu_vs
    frames = _clip(16, 7)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    n = walk(vs, lambda: vs.Stabilizer(device=0, lag=4, smoother_memory=2, crop_pixels=8, border_fill=3), call, 17, throwing)
    print("filled process_batch: %d allocations failed one by one (%s)" % (n, "throwing" if throwing else "error code"))


def test_video_test_fill_writes_what_the_library_returns(gpu_vs, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    frames = _clip(40, 77)
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    r = subprocess.run([os.path.join(ROOT, "apps", "bin", "vs_video_test"), str(d), str(tmp_path / "out"), "--crop", "0", "--fill", "4", "--chunk", "13"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = gpu_vs.Stabilizer(device=0, crop_pixels=0, border_fill=4)
    want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_" + raw.name), np.uint8).reshape(-1, H, W, 3)
    assert np.array_equal(got, want)
    plain = gpu_vs.Stabilizer(device=0, crop_pixels=0)
    assert not np.array_equal(want, np.stack([o for o in (plain.process(f) for f in frames) if o is not None]))
    r = subprocess.run([os.path.join(ROOT, "apps", "bin", "vs_video_test"), str(d), str(tmp_path / "out2"), "--fill", "4", "--lanczos2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "vs_stabilizer_set_border_fill" in r.stderr
