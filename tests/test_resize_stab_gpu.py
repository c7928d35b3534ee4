"""The output size in the stabilizer (include/vs_amd.h: vs_stabilizer_set_output_size) on 160 x 128 clips of a dozen frames: off is the handle
as it was; on, every output equals vs_bgr_resize_batch applied to what the handle with the pass off returns -- whatever the chunking,
scheduling, memory, format, warp mode and the passes in front of it; the scratch may go in any number of groups; the YCbCr wrapper equals its
three calls; a window that already has the requested size launches nothing; a refusal leaves the state alone.  Bit for bit throughout."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from _stab_routes import batches, frame_by_frame, same, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, LAG = 160, 128, 14, 4
KW = dict(device=0, lag=LAG, crop_pixels=8)
SIZES = [((-1, -1), (W, H)), ((96, 64), (96, 64))]           # what is set, what is delivered


def _clip(n=N, seed=3, bits=8, **kw):
    from video_stabilizer_amd import synth
    return np.maximum(synth.make_clip(W, H, n, seed=seed, channels=3, bits=bits, **dict(dict(pan=1.0, jitter_t=2.0), **kw))[0], 1)


@pytest.fixture(scope="module")
def clip8():
    return _clip()


def _want(vs, frames, size, filt, fmt=None, **kw):
    """{k: vs_bgr_resize_batch of the off handle's output k}, and the off handle's states"""
    states = []
    off = frame_by_frame(vs.Stabilizer(**dict(KW, **kw)), frames, states)
    return {k: vs.resize_batch(off[k][None], size[0], size[1], filt, fmt=fmt)[0] for k in off}, off, states


def test_off_is_the_handle_that_was(gpu_vs, clip8):
    vs = gpu_vs
    never, null = vs.Stabilizer(**KW), vs.Stabilizer(**KW)
    null.set_output_size(96, 64, vs.RESIZE_AREA)
    assert null.get_output_size() == (96, 64, vs.RESIZE_AREA) and null.delivered_size(W, H) == (96, 64)
    null.set_output_size(0, 0)
    assert never.get_output_size() is None and null.get_output_size() is None and null.delivered_size(W, H) == (W - 16, H - 16)
    assert vs.Stabilizer(output_size=(-1, -1), **KW).get_output_size() == (-1, -1, vs.RESIZE_LINEAR)
    s0, s1 = [], []
    assert same(frame_by_frame(never, clip8, s0), frame_by_frame(null, clip8, s1)) and s0 == s1

    # allocation for allocation: switched on and off again is never switched on; on: the scratch block more.  A window that already has the
    # requested size is off: nothing launched (the same bytes), nothing allocated
    def allocations(make):
        s = make()
        vs.test_fail_alloc(1 << 30)
        out, has = s.process_batch(clip8)
        return vs.test_fail_alloc(0), out, has

    def switched():
        s = vs.Stabilizer(**KW)
        s.set_output_size(-1, -1)
        s.set_output_size(0, 0)
        return s
    allocations(lambda: vs.Stabilizer(**KW))                 # (process-wide: the staging pool and the calling thread's rings fill on first use)
    allocations(lambda: vs.Stabilizer(output_size=(-1, -1), **KW))
    n_never, out_never, has_never = allocations(lambda: vs.Stabilizer(**KW))
    n_null, out_null, has_null = allocations(switched)
    n_same, out_same, has_same = allocations(lambda: vs.Stabilizer(output_size=(W - 16, H - 16, vs.RESIZE_AREA), **KW))
    n_on, out_on, has_on = allocations(lambda: vs.Stabilizer(output_size=(-1, -1), **KW))
    assert n_null == n_never and has_null == has_never and np.array_equal(out_null, out_never)
    assert n_same == n_never and has_same == has_never and np.array_equal(out_same, out_never)
    assert n_on == n_never + 1 and has_on == has_never and out_on.shape == (N, H, W, 3)


@pytest.mark.parametrize("size,delivered", SIZES, ids=["source", "96x64"])
def test_on_is_the_resize_of_the_off_handle_on_every_route(gpu_vs, clip8, size, delivered):
    """frame by frame == process_batch in one call and in calls of 5 and 13 == device memory == process_clips; the state is the off handle's"""
    import torch
    vs = gpu_vs
    dw, dh = delivered
    for filt in (vs.RESIZE_LINEAR,) + ((vs.RESIZE_AREA,) if dw <= W - 16 else ()):
        want, off, s_off = _want(vs, clip8, delivered, filt)
        assert len(want) == N - LAG and all(v.shape == (dh, dw, 3) for v in want.values())
        kw = dict(KW, output_size=size + (filt,))
        s_on = []
        assert same(frame_by_frame(vs.Stabilizer(**kw), clip8, s_on), want)
        assert s_on == s_off                                 # transforms, state and has_output are left alone
        assert same(batches(vs.Stabilizer(**kw), clip8, (N,)), want)
        assert same(batches(vs.Stabilizer(**kw), clip8, (5,)), want)
        assert same(batches(vs.Stabilizer(**kw), clip8, (13, 1)), want)
        dev = torch.from_numpy(clip8).cuda()
        dout = torch.zeros((N, dh, dw, 3), dtype=torch.uint8, device="cuda")
        st = vs.Stabilizer(**kw)
        r, hs = st.process_batch_device(dev.data_ptr(), N, W, H, vs.FMT_BGR8, dout.data_ptr())
        torch.cuda.synchronize()
        res = dout.cpu().numpy()
        assert r == len(want) and same({i - LAG: res[i] for i, hh in enumerate(hs) if hh}, want)
    # two clips through process_clips, host and device memory: each equals the clip on a handle of its own
    second = _clip(seed=9)
    want2, _, _ = _want(vs, second, delivered, filt)
    two = np.concatenate([clip8, second])
    out, has = vs.Stabilizer(**kw).process_clips(two, 2)
    dtwo = torch.from_numpy(two).cuda()
    dout2 = torch.zeros((2 * N, dh, dw, 3), dtype=torch.uint8, device="cuda")
    r, dhas = vs.Stabilizer(**kw).process_clips_device(dtwo.data_ptr(), 2, N, W, H, vs.FMT_BGR8, dout2.data_ptr())
    torch.cuda.synchronize()
    res2 = dout2.cpu().numpy()
    assert has == dhas and sum(has) == 2 * (N - LAG)
    for c, wn in enumerate((want, want2)):
        for i in range(N):
            if has[c * N + i]:
                assert np.array_equal(out[c * N + i], wn[i - LAG]) and np.array_equal(res2[c * N + i], wn[i - LAG]), (c, i)


def test_behind_fill_inpaint_sharpen_and_deflicker(gpu_vs):
    """every pass that writes the window, then the deflicker's gain, then the resize: the off handle with the same passes, resized"""
    vs = gpu_vs
    frames = _clip(16, 5, pan=2.0, jitter_t=4.0).astype(np.float64)
    frames = np.clip(frames * (0.8 + 0.15 * np.sin(np.arange(16) * 1.3))[:, None, None, None], 1, 255).astype(np.uint8)
    extra = dict(crop_pixels=8, border_fill=3, inpaint=1, sharpen=True, deflicker=3, deblur=2, denoise=2)
    for size, delivered in SIZES:
        want, off, _ = _want(vs, frames, delivered, vs.RESIZE_LINEAR, **extra)
        plain = frame_by_frame(vs.Stabilizer(**KW), frames)
        assert not same(off, plain)                         # premise: the passes did something
        assert same(frame_by_frame(vs.Stabilizer(**dict(KW, output_size=size, **extra)), frames), want)
        assert same(batches(vs.Stabilizer(**dict(KW, output_size=size, **extra)), frames, (5, 13)), want)


@pytest.mark.parametrize("mode", ["WARP_LANCZOS2", "WARP_LANCZOS2_FAST", "WARP_BILINEAR"])
def test_the_other_warp_modes(gpu_vs, clip8, mode):
    vs = gpu_vs
    extra = dict(warp_mode=getattr(vs, mode))
    want, _, _ = _want(vs, clip8, (W, H), vs.RESIZE_LINEAR, **extra)
    assert same(batches(vs.Stabilizer(**dict(KW, output_size=(-1, -1), **extra)), clip8, (N,)), want)
    assert same(frame_by_frame(vs.Stabilizer(**dict(KW, output_size=(-1, -1), **extra)), clip8), want)


def test_ten_bit(gpu_vs):
    vs = gpu_vs
    frames = _clip(bits=10)
    assert frames.dtype == np.uint16 and frames.max() > 255
    for size, delivered in SIZES:
        want, off, _ = _want(vs, frames, delivered, vs.RESIZE_LINEAR, fmt=vs.FMT_BGR10)
        assert max(int(v.max()) for v in want.values()) > 255
        kw = dict(KW, output_size=size)
        assert same(frame_by_frame(vs.Stabilizer(**kw), frames), want)
        assert same(batches(vs.Stabilizer(**kw), frames, (5,), fmt=vs.FMT_BGR10), want)


@pytest.mark.parametrize("lag", [0, 6])
def test_lag_0_and_6(gpu_vs, clip8, lag):
    vs = gpu_vs
    for size, delivered in SIZES:
        want, _, _ = _want(vs, clip8, delivered, vs.RESIZE_AREA if delivered[0] < W - 16 else vs.RESIZE_LINEAR, lag=lag)
        assert len(want) == N - lag
        kw = dict(KW, lag=lag, output_size=size + (vs.RESIZE_AREA if delivered[0] < W - 16 else vs.RESIZE_LINEAR,))
        assert same(frame_by_frame(vs.Stabilizer(**kw), clip8), want)
        assert same(batches(vs.Stabilizer(**kw), clip8, (13, 1)), want)


def test_the_ycbcr_wrapper_equals_its_three_calls(gpu_vs, clip8):
    """planes in, planes out at the delivered size: vs_ycbcr_to_bgr_batch, the stabilizer with the output size set, vs_bgr_to_ycbcr_batch"""
    vs = gpu_vs
    y, cb, cr = vs.bgr_to_ycbcr_batch(clip8)
    bgr = vs.ycbcr_to_bgr_batch(y, cb, cr)
    for size, delivered in SIZES:
        kw = dict(KW, output_size=size)
        out, has = vs.Stabilizer(**kw).process_batch(bgr)
        (gy, gcb, gcr), ghas = vs.Stabilizer(**kw).process_batch_ycbcr(y, cb, cr)
        assert ghas == has and gy.shape == (N, delivered[1], delivered[0])
        live = np.array(has, bool)
        wy, wcb, wcr = vs.bgr_to_ycbcr_batch(out[live])
        assert np.array_equal(gy[live], wy) and np.array_equal(gcb[live], wcb) and np.array_equal(gcr[live], wcr)


def test_refusals_leave_the_state_alone(gpu_vs, clip8):
    vs = gpu_vs
    st = vs.Stabilizer(**KW)
    for bad in ((0, 5), (5, 0), (-1, 5), (-2, -2), (5, -1)):
        with pytest.raises(vs.VsError, match="error -1"):
            st.set_output_size(*bad)
    with pytest.raises(vs.VsError, match="error -1"):
        st.set_output_size(96, 64, 2)
    for big in ((32768, 64), (96, 32768)):
        with pytest.raises(vs.VsError, match="error -3.*32767"):
            st.set_output_size(*big)
    assert st.get_output_size() is None
    # AREA cannot enlarge, nor shrink past 8:1: the call is refused before any work; queue, smoother and state stay as they were
    want, _, s_off = _want(vs, clip8, (96, 64), vs.RESIZE_AREA)
    st.set_output_size(96, 64, vs.RESIZE_AREA)
    got, states = {}, []
    for i, f in enumerate(clip8):
        if i == 7:
            before = tuple(x.tup() if hasattr(x, "tup") else x for x in st.state())
            st.set_output_size(-1, -1, vs.RESIZE_AREA)       # the window is smaller than the source size
            with pytest.raises(vs.VsError, match="error -3.*x axis"):
                st.process(f)
            st.set_output_size(17, 64, vs.RESIZE_AREA)       # 144 > 8 * 17
            with pytest.raises(vs.VsError, match="error -3.*x axis"):
                st.process(f)
            st.set_output_size(96, 13, vs.RESIZE_AREA)       # 112 > 8 * 13
            with pytest.raises(vs.VsError, match="error -3.*y axis"):
                st.process_batch(clip8[i:i + 3])
            assert tuple(x.tup() if hasattr(x, "tup") else x for x in st.state()) == before
            st.set_output_size(96, 64, vs.RESIZE_AREA)
        o = st.process(f)
        m, a, s = st.state()
        states.append((m.tup(), a.tup(), s, o is not None))
        if o is not None:
            got[i - LAG] = o
    assert same(got, want) and states == s_off


def test_reset_and_a_size_change(gpu_vs, clip8):
    vs = gpu_vs
    want, _, _ = _want(vs, clip8, (W, H), vs.RESIZE_LINEAR)
    st = vs.Stabilizer(output_size=(-1, -1), **KW)
    frame_by_frame(st, _clip(seed=11))
    st.reset()
    assert st.get_output_size() == (-1, -1, vs.RESIZE_LINEAR)            # the size is a setting, not state
    assert same(frame_by_frame(st, clip8), want)
    # frames of another size: a new clip, delivered at ITS source size; then a fixed size mid-clip takes effect with the next call
    from video_stabilizer_amd import synth
    other = np.maximum(synth.make_clip(192, 144, N, seed=4, channels=3, pan=1.0, jitter_t=2.0)[0], 1)
    off = frame_by_frame(vs.Stabilizer(**KW), other)
    on = frame_by_frame(st, other)
    assert same(on, {k: vs.resize_batch(off[k][None], 192, 144)[0] for k in off})
    st2, got = vs.Stabilizer(**KW), {}
    off8 = frame_by_frame(vs.Stabilizer(**KW), clip8)
    for i, f in enumerate(clip8):
        if i == 8:
            st2.set_output_size(200, 150)
        o = st2.process(f)
        if o is not None:
            got[i - LAG] = o
    assert same(got, {k: (off8[k] if k + LAG < 8 else vs.resize_batch(off8[k][None], 200, 150)[0]) for k in off8})


CHILD = r'''
import sys, hashlib, os
sys.path.insert(0, %r)
import numpy as np, torch
from video_stabilizer_amd import capi, synth
W, H, crop, n = 160, 128, 8, 144
frames = np.maximum(synth.make_clip(W, H, n, seed=3, channels=3, pan=1.0, jitter_t=2.0)[0], 1)
dev = torch.from_numpy(frames).cuda()
out = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
kw = dict(device=0, lag=4, crop_pixels=crop, sharpen=True, output_size=(-1, -1))
st = capi.Stabilizer(**kw)
r, has = st.process_batch_device(dev.data_ptr(), n, W, H, capi.FMT_BGR8, out.data_ptr())
torch.cuda.synchronize()
res = [str(r), hashlib.sha256(out.cpu().numpy().tobytes() + bytes(has)).hexdigest()]
hout, hhas = capi.Stabilizer(**kw).process_batch(frames[:40])
res.append(hashlib.sha256(hout.tobytes() + bytes(hhas)).hexdigest())
print("DIGEST", *res)
'''


def test_every_scheduling_switch_and_scratch_budget_gives_the_same_bytes(gpu_vs):
    """one device-resident take of 144 frames, long enough for the overlapped run path to cut it in time: the warps, and the resize behind
    them, go to a second stream under the next chunk's alignment.  And a host batch of 40 frames.  The switches and the gate of the scratch
    budget's test hook are read once per process: one child each, the budgets spread over them -- the default (one group), one window (a group
    per frame), three windows, seven"""
    vs = gpu_vs
    crop, n = 8, 144
    frames = _clip(n)
    st = vs.Stabilizer(sharpen=True, output_size=(-1, -1), **KW)
    outs, has = [], []
    for f in frames:
        o = st.process(f)
        has.append(1 if o is not None else 0)
        outs.append(o if o is not None else np.zeros((H, W, 3), np.uint8))
    outs = np.stack(outs)
    want = [str(n - LAG), hashlib.sha256(outs.tobytes() + bytes(has)).hexdigest(), hashlib.sha256(outs[:40].tobytes() + bytes(has[:40])).hexdigest()]
    window = (W - 2 * crop) * (H - 2 * crop) * 3
    for env, budget in (({"VS_STAB_OVERLAP": "1", "VS_STAB_PREFETCH": "1"}, None), ({"VS_STAB_OVERLAP": "1", "VS_STAB_PREFETCH": "0"}, window),
                        ({"VS_STAB_OVERLAP": "0"}, 3 * window + 5), ({"VS_STAB_OVERLAP": "1", "VS_STAB_PREFETCH": "1", "VS_GN_CORESIDENT": "0"}, 7 * window)):
        env = dict(os.environ, VS_TEST_HOOKS="1", **env)
        env.pop("VS_TEST_RESIZE_SCRATCH_BYTES", None)
        if budget is not None:
            env["VS_TEST_RESIZE_SCRATCH_BYTES"] = str(budget)
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1].split()[1:]
        assert line == want, (env.get("VS_TEST_RESIZE_SCRATCH_BYTES"), line, want)


@pytest.mark.parametrize("throwing", [False, True])
def test_resized_process_batch_survives_every_allocation_failure(gpu_vs, clip8, throwing):
    vs = gpu_vs

    def call(s):
        out, has = s.process_batch(clip8)
        return list(has), out.tobytes()
    kw = dict(KW, smoother_memory=2, sharpen=True, deflicker=2)

    def allocations(make):
        h = make()
        vs.test_fail_alloc(1 << 30)
        call(h)
        return vs.test_fail_alloc(0)
    allocations(lambda: vs.Stabilizer(output_size=(-1, -1), **kw))       # (the process-wide staging pool and rings fill on the first call)
    n_off, n_on = allocations(lambda: vs.Stabilizer(**kw)), allocations(lambda: vs.Stabilizer(output_size=(-1, -1), **kw))
    assert n_on == n_off + 1                                             # the scratch block joins the protocol
    fired = walk(vs, lambda: vs.Stabilizer(output_size=(-1, -1), **kw), call, n_on, throwing)
    assert fired == n_on
