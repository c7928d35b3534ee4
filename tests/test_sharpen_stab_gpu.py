"""Phase-compensated sharpening in the stabilizer (include/vs_amd.h: vs_stabilizer_set_sharpen) on 160 x 128 clips of a dozen frames: off is the
handle as it was; on, every output equals the kernel-level sequence -- the stabilizer's output with sharpen off, then vs_bgr_sharpen_batch under
that frame's own correction -- whatever the chunking, scheduling, memory, format and the passes around it; the deflicker's gain stays last; the
scratch may go in any number of groups; every allocation may fail.  Bit for bit throughout."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import _sharpen_ref as R
from _stab_routes import batches, frame_by_frame, same, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N, LAG = 160, 128, 14, 4
KW = dict(device=0, lag=LAG, crop_pixels=8)


def _clip(n=N, seed=3, bits=8, **kw):
    """a hand-held camera the aligner follows at every step; no zero samples, so that a black border cannot coincide with a sample"""
    from video_stabilizer_amd import synth
    return np.maximum(synth.make_clip(W, H, n, seed=seed, channels=3, bits=bits, **dict(dict(pan=1.0, jitter_t=2.0), **kw))[0], 1)


@pytest.fixture(scope="module")
def clip8():
    return _clip()


def _sequence(vs, frames, fmt=None, **kw):
    """-> ({k: output with sharpen off}, {k: the kernel-level sequence on it}, {k: correction}): the off handle frame by frame, its state after each
    output -- the accumulated correction of the frame just put out -- and vs_bgr_sharpen_batch under the inverse of it, the transform of that
    frame's warp job"""
    kw = dict(KW, **kw)
    crop = kw["crop_pixels"]
    strength = kw.pop("strength", 16)
    st = vs.Stabilizer(**kw)
    states = []
    off = frame_by_frame(st, frames, states)
    corr = {i - kw["lag"]: vs.t_inverse(vs.Transform.of(*a)) for i, (_, a, _, has) in enumerate(states) if has}
    assert sorted(corr) == sorted(off)
    want = {k: vs.sharpen_batch(off[k][None], [corr[k]], W, H, crop, crop, params=vs.sharpen_params(strength=strength), fmt=fmt)[0] for k in off}
    return off, want, corr


def test_off_is_the_handle_that_was(gpu_vs, clip8):
    vs = gpu_vs
    never, null = vs.Stabilizer(**KW), vs.Stabilizer(**KW)
    null.set_sharpen(vs.sharpen_params(strength=24))
    assert null.get_sharpen().strength == 24
    null.set_sharpen(None)
    assert never.get_sharpen() is None and null.get_sharpen() is None
    assert vs.Stabilizer(sharpen=True, **KW).get_sharpen().strength == 16
    s0, s1 = [], []
    assert same(frame_by_frame(never, clip8, s0), frame_by_frame(null, clip8, s1)) and s0 == s1

    # allocation for allocation: a handle that had the pass switched on and off again allocates what one that never had it does; on: one block more
    def allocations(make):
        s = make()
        vs.test_fail_alloc(1 << 30)
        out, has = s.process_batch(clip8)
        return vs.test_fail_alloc(0), out, has

    def switched():
        s = vs.Stabilizer(**KW)
        s.set_sharpen(vs.sharpen_params())
        s.set_sharpen(None)
        return s
    # (process-wide and not the handle's: the staging pool fills on the first call, and the calling thread's parameter ring, which brings the
    # sharpen its matrices and which a plain warp of so few frames never touches, on the first call that uses it)
    allocations(lambda: vs.Stabilizer(**KW))
    allocations(lambda: vs.Stabilizer(sharpen=True, **KW))
    n_never, out_never, has_never = allocations(lambda: vs.Stabilizer(**KW))
    n_null, out_null, has_null = allocations(switched)
    n_on, out_on, has_on = allocations(lambda: vs.Stabilizer(sharpen=True, **KW))
    assert n_null == n_never and has_null == has_never and np.array_equal(out_null, out_never)
    assert n_on == n_never + 1 and has_on == has_never and not np.array_equal(out_on, out_never)


@pytest.mark.parametrize("strength", [16, 32])
def test_on_is_the_kernel_level_sequence_on_every_route(gpu_vs, clip8, strength):
    """frame by frame == process_batch in one call and in split calls == device memory == process_clips; the state is the off handle's"""
    import torch
    vs = gpu_vs
    off, want, corr = _sequence(vs, clip8, strength=strength)
    changed = sum(int((want[k] != off[k]).any(-1).sum()) for k in off)
    # premise: sub-pixel corrections; the clip is flat patches with edges between them, and every tenth pixel lies at one
    assert len(off) == N - LAG and changed > 0.1 * len(off) * (W - 16) * (H - 16)
    # premise: the restatement agrees with the kernel-level call here (tests/test_sharpen_gpu.py is about that)
    k0 = sorted(off)[2]
    assert np.array_equal(want[k0], R.sharpen(vs, off[k0], corr[k0], W, H, (8, 8, W - 16, H - 16), strength, 255))
    kw = dict(KW, sharpen=vs.sharpen_params(strength=strength))
    s_on, s_off = [], []
    assert same(frame_by_frame(vs.Stabilizer(**kw), clip8, s_on), want)
    frame_by_frame(vs.Stabilizer(**KW), clip8, s_off)
    assert s_on == s_off                                                 # transforms, state and has_output are left alone
    assert same(batches(vs.Stabilizer(**kw), clip8, (N,)), want)
    assert same(batches(vs.Stabilizer(**kw), clip8, (3, 1, 5, 2)), want)
    dev = torch.from_numpy(clip8).cuda()
    dout = torch.zeros((N, H - 16, W - 16, 3), dtype=torch.uint8, device="cuda")
    r, hs = vs.Stabilizer(**kw).process_batch_device(dev.data_ptr(), N, W, H, vs.FMT_BGR8, dout.data_ptr())
    torch.cuda.synchronize()
    res = dout.cpu().numpy()
    assert r == len(want) and same({i - LAG: res[i] for i, hh in enumerate(hs) if hh}, want)
    # two clips through process_clips: each equals the clip on a handle of its own
    second = _clip(seed=9)
    off2, want2, _ = _sequence(vs, second, strength=strength)
    two = np.concatenate([clip8, second])
    out, has = vs.Stabilizer(**kw).process_clips(two, 2)
    dtwo = torch.from_numpy(two).cuda()
    dout2 = torch.zeros((2 * N, H - 16, W - 16, 3), dtype=torch.uint8, device="cuda")
    r, dhas = vs.Stabilizer(**kw).process_clips_device(dtwo.data_ptr(), 2, N, W, H, vs.FMT_BGR8, dout2.data_ptr())
    torch.cuda.synchronize()
    res2 = dout2.cpu().numpy()
    assert has == dhas and sum(has) == 2 * (N - LAG)
    for c, wn in enumerate((want, want2)):
        for i in range(N):
            if has[c * N + i]:
                assert np.array_equal(out[c * N + i], wn[i - LAG]) and np.array_equal(res2[c * N + i], wn[i - LAG]), (c, i)


def test_ten_bit(gpu_vs):
    vs = gpu_vs
    frames = _clip(bits=10)
    assert frames.dtype == np.uint16 and frames.max() > 255
    off, want, _ = _sequence(vs, frames, fmt=vs.FMT_BGR10)
    assert not same(off, want)
    kw = dict(KW, sharpen=True)
    assert same(frame_by_frame(vs.Stabilizer(**kw), frames), want)     # (uint16 numpy frames are 10-bit unless the caller says otherwise)
    out, has = vs.Stabilizer(**kw).process_batch(frames, fmt=vs.FMT_BGR10)
    assert same({i - LAG: out[i] for i, hh in enumerate(has) if hh}, want)


def test_fill_and_inpaint_pixels_are_unchanged_at_crop_0(gpu_vs, clip8):
    """crop 0 with fill and inpaint: the sharpen reads the window as those passes leave it, and what the frame's own source does not cover -- fill
    and inpaint pixels -- and its edge neighbours come back as they were"""
    vs = gpu_vs
    frames = _clip(20, 5, pan=2.0, jitter_t=4.0)
    extra = dict(crop_pixels=0, border_fill=3, inpaint=1)
    off, want, corr = _sequence(vs, frames, **extra)
    on = frame_by_frame(vs.Stabilizer(**dict(KW, sharpen=True, **extra)), frames)
    assert same(on, want)
    plain = frame_by_frame(vs.Stabilizer(**dict(KW, crop_pixels=0)), frames)
    open_px = kept = 0
    for k in off:
        X, Y = R.positions(vs, corr[k], W, H)
        cov = R.covered(X, Y, W, H)
        near = ~cov
        near[1:] |= ~cov[:-1]; near[:-1] |= ~cov[1:]; near[:, 1:] |= ~cov[:, :-1]; near[:, :-1] |= ~cov[:, 1:]
        assert np.array_equal(on[k][near], off[k][near]), k
        open_px += int((~cov).sum())
        kept += int((off[k][~cov] != plain[k][~cov]).any(-1).sum())
    assert open_px > 2000 and kept > 0.9 * open_px                       # premise: there was a rim, and fill and inpaint had written it


def test_the_deflickers_gain_stays_last(gpu_vs):
    """with deflicker on the output is gain(sharpen(warp)).  The gain is a per-frame, per-channel map of sample values: read off the two sharpen-off
    outputs (without and with deflicker), it must take the sharpen-only output to the output with both on wherever the value occurs"""
    vs = gpu_vs
    frames = _clip(16, 5).astype(np.float64)
    frames = np.clip(frames * (0.8 + 0.15 * np.sin(np.arange(16) * 1.3))[:, None, None, None], 1, 255).astype(np.uint8)
    w_ = frame_by_frame(vs.Stabilizer(**KW), frames)                                   # warp
    y_ = frame_by_frame(vs.Stabilizer(deflicker=3, **KW), frames)                      # gain(warp)
    z_ = frame_by_frame(vs.Stabilizer(sharpen=True, **KW), frames)                     # sharpen(warp)
    x_ = frame_by_frame(vs.Stabilizer(sharpen=True, deflicker=3, **KW), frames)        # both
    checked = scaled = 0
    for k in w_:
        for c in range(3):
            table = np.full(256, -1, np.int64)
            table[w_[k][..., c]] = y_[k][..., c]
            assert np.array_equal(table[w_[k][..., c]], y_[k][..., c])                  # one map per channel: the premise
            zi = z_[k][..., c]
            known = table[zi] >= 0
            assert np.array_equal(x_[k][..., c][known], table[zi][known]), (k, c)
            checked += int(known.sum())
            scaled += int((table[zi][known] != zi[known]).sum())
    assert checked > 100000 and scaled > 1000
    assert not same(z_, w_) and not same(x_, y_)


def test_reset_and_refusals(gpu_vs, clip8):
    vs = gpu_vs
    _, want, _ = _sequence(vs, clip8)
    st = vs.Stabilizer(sharpen=True, **KW)
    frame_by_frame(st, _clip(seed=11))
    st.reset()
    assert st.get_sharpen().strength == 16                               # the switch is a setting, not state
    assert same(frame_by_frame(st, clip8), want)
    # a Lanczos2 handle is refused with the fill's wording; a strength outside 1 .. 32 is an argument error and leaves the setting alone
    lz = vs.Stabilizer(warp_mode=vs.WARP_LANCZOS2_FAST, **KW)
    with pytest.raises(vs.VsError, match="error -3.*sharpen: VS_WARP_BILINEAR_CV handles only"):
        lz.set_sharpen(vs.sharpen_params())
    with pytest.raises(vs.VsError, match="error -3"):
        lz.set_sharpen(None)
    for s in (0, 33, -16):
        with pytest.raises(vs.VsError, match="error -1"):
            st.set_sharpen(vs.sharpen_params(strength=s))
    assert st.get_sharpen().strength == 16


CHILD = r'''
import sys, hashlib, os
sys.path.insert(0, %r)
import numpy as np, torch
from video_stabilizer_amd import capi, synth
W, H, crop, n = 160, 128, 8, 144
frames = np.maximum(synth.make_clip(W, H, n, seed=3, channels=3, pan=1.0, jitter_t=2.0)[0], 1)
dev = torch.from_numpy(frames).cuda()
out = torch.zeros((n, H - 2 * crop, W - 2 * crop, 3), dtype=torch.uint8, device="cuda")
st = capi.Stabilizer(device=0, lag=4, crop_pixels=crop, sharpen=True)
r, has = st.process_batch_device(dev.data_ptr(), n, W, H, capi.FMT_BGR8, out.data_ptr())
torch.cuda.synchronize()
res = [str(r), hashlib.sha256(out.cpu().numpy().tobytes() + bytes(has)).hexdigest()]
hout, hhas = capi.Stabilizer(device=0, lag=4, crop_pixels=crop, sharpen=True).process_batch(frames[:40])
res.append(hashlib.sha256(hout.tobytes() + bytes(hhas)).hexdigest())
print("DIGEST", *res)
'''


def test_every_scheduling_switch_and_scratch_budget_gives_the_same_bytes(gpu_vs):
    """one device-resident take of 144 frames, long enough for the overlapped run path to cut it in time (the default warp: chunks of 120): the
    warps, and the sharpen behind them, go to a second stream under the next chunk's alignment.  And a host batch of 40 frames.  Every switch
    tests/test_stab_modes_gpu.py walks is read once per process, and so is the gate of the scratch budget's test hook: one child each, the
    budgets spread over them -- the default (one group), one window (a group per frame), three windows, seven"""
    vs = gpu_vs
    crop, n = 8, 144
    frames = _clip(n)
    st = vs.Stabilizer(sharpen=True, **KW)
    outs, has = [], []
    for f in frames:
        o = st.process(f)
        has.append(1 if o is not None else 0)
        outs.append(o if o is not None else np.zeros((H - 2 * crop, W - 2 * crop, 3), np.uint8))
    outs = np.stack(outs)
    want = [str(n - LAG), hashlib.sha256(outs.tobytes() + bytes(has)).hexdigest(), hashlib.sha256(outs[:40].tobytes() + bytes(has[:40])).hexdigest()]
    window = (W - 2 * crop) * (H - 2 * crop) * 3
    for env, budget in (({"VS_STAB_OVERLAP": "1", "VS_STAB_PREFETCH": "1"}, None), ({"VS_STAB_OVERLAP": "1", "VS_STAB_PREFETCH": "0"}, window),
                        ({"VS_STAB_OVERLAP": "0"}, 3 * window + 5), ({"VS_STAB_OVERLAP": "1", "VS_STAB_PREFETCH": "1", "VS_GN_CORESIDENT": "0"}, 7 * window)):
        env = dict(os.environ, VS_TEST_HOOKS="1", **env)
        env.pop("VS_TEST_SHARPEN_SCRATCH_BYTES", None)
        if budget is not None:
            env["VS_TEST_SHARPEN_SCRATCH_BYTES"] = str(budget)
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1].split()[1:]
        assert line == want, (env.get("VS_TEST_SHARPEN_SCRATCH_BYTES"), line, want)


def test_video_test_sharpen_writes_what_the_library_returns(gpu_vs, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    frames = _clip(20, 77)
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    exe = os.path.join(ROOT, "apps", "bin", "vs_video_test")
    for args, params in ((["--sharpen"], gpu_vs.sharpen_params()), (["--sharpen", "24"], gpu_vs.sharpen_params(strength=24))):
        out = tmp_path / ("out%d" % params.strength)
        r = subprocess.run([exe, str(d), str(out), "--crop", "8", "--chunk", "7"] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        st = gpu_vs.Stabilizer(device=0, crop_pixels=8, sharpen=params)
        want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
        got = np.fromfile(out / ("processed_" + raw.name), np.uint8).reshape(-1, H - 16, W - 16, 3)
        assert np.array_equal(got, want)
    for args in (["--sharpen", "--lanczos2"], ["--sharpen", "0"], ["--sharpen", "33"]):
        r = subprocess.run([exe, str(d), str(tmp_path / "bad")] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "vs_stabilizer_set_sharpen" in r.stderr, args


@pytest.mark.parametrize("throwing", [False, True])
def test_sharpened_process_batch_survives_every_allocation_failure(gpu_vs, clip8, throwing):
    vs = gpu_vs

    def call(s):
        out, has = s.process_batch(clip8)
        return list(has), out.tobytes()
    kw = dict(KW, smoother_memory=2, border_fill=2, inpaint=1, deflicker=2, crop_pixels=0)

    def allocations(make):
        h = make()
        vs.test_fail_alloc(1 << 30)
        call(h)
        return vs.test_fail_alloc(0)
    allocations(lambda: vs.Stabilizer(**kw))                             # (the process-wide staging pool fills on the first call)
    n_off, n_on = allocations(lambda: vs.Stabilizer(**kw)), allocations(lambda: vs.Stabilizer(sharpen=True, **kw))
    assert n_on == n_off + 1                                             # the scratch block joins the protocol
    fired = walk(vs, lambda: vs.Stabilizer(sharpen=True, **kw), call, n_on, throwing)
    print("sharpened process_batch: %d allocations failed one by one (%s)" % (fired, "throwing" if throwing else "error code"))
    assert fired == n_on
