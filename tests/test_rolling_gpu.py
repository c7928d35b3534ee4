"""Rolling-shutter correction on the GPU (include/vs_amd.h: vs_bgr_rolling_batch, vs_stabilizer_set_rolling_shutter) against the rule's
restatement (tests/_rolling_ref.py).  Kernel level: np.array_equal -- the rule fixes every bit.  Engine level: the engine against the engine
model on the CPU oracle's transforms, np.array_equal; the pass off against a handle that never heard of it; the direction test through the
C ABI."""
import numpy as np
import pytest

import _denoise_ref as DN
import _engine_model as EM
import _hostile_maps as HM
import _inpaint_ref as IP
import _rolling_ref as R
from _stab_routes import frame_by_frame
from test_rolling_cpu import direction_errors

pytestmark = pytest.mark.gpu

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr16": (4, np.uint16, 16)}
# a frame smaller than a wave; strip (8 rows) and workgroup (64 x 32, 256 x 32) seams; widths that take the four-pixel form (64, 260) and
# widths that refuse it
SHAPES = [(1, 1), (3, 2), (63, 5), (64, 8), (65, 9), (257, 33), (260, 32)]
RHOS = (-1.0, 0.0, 0.5, 1.0)
MOTIONS = [(0.0, 0.0, 7.0, -3.0), (0.02, -0.03, 2.5, 1.25), (-0.01, 0.015, -4.0, 6.5), (0.0, 0.0, 0.0, 0.0)]


def _noise(rng, n, w, h, dtype, maxv):
    return rng.integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)


def _lists(vs, rng):
    """four output frames, with and without a motion in one batch; entry 1's index is only looked at for its sign (7: no such frame)"""
    cf = np.array([[0, 1], [1, -1], [2, 7], [0, 0]], np.int32)
    ct = [[vs.Transform.of(*rng.uniform(-1, 1, 4)), vs.Transform.of(*MOTIONS[i])] for i in range(4)]
    ct[3][1] = vs.Transform.of(rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-6, 6), rng.uniform(-6, 6))
    return cf, ct


def _want(vs, src, cf, ct, rho, maxv):
    return R.rolling_batch(HM.cvinv(vs), src, cf, ct, rho, maxv)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_rolling_batch_equals_the_rule(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(100 + bits)
    guard = 0x5A if bits == 8 else 0x5A5A
    moved = 0
    for w, h in SHAPES:
        src = _noise(rng, 3, w, h, dtype, maxv)
        cf, ct = _lists(vs, rng)
        for rho in RHOS:
            p = vs.rolling_params(readout=rho)
            want = _want(vs, src, cf, ct, rho, maxv)
            assert np.array_equal(want[1], src[1])                   # (a) no motion
            moved += int((want != src[cf[:, 0]]).sum())
            got = vs.rolling_batch(src, cf, ct, params=p, fmt=code)
            assert np.array_equal(got, want), (w, h, rho, int((got != want).sum()))
            # n_out == 1
            assert np.array_equal(vs.rolling_batch(src, cf[3:], ct[3:], params=p, fmt=code), want[3:]), (w, h, rho)
            if rho != 0.5:
                continue
            # pitched rows on both sides: odd (the destination's rows leave the dwords: the one-pixel form), then rows that start on dwords;
            # the destination's padding must stay untouched
            for ss, ds in ((3 * w + 7, 3 * w + 5), (3 * w + 8, 3 * w + 4)):
                res, padded = vs.rolling_batch(src, cf, ct, params=p, fmt=code, src_stride=ss, dst_stride=ds, guard=guard)
                assert np.array_equal(res, want), (w, h, ss, ds)
                assert (padded[:, :, 3 * w:] == guard).all()
    assert moved > 10000                                             # the comparison was about resampled frames


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_the_rule_s_consequences_on_the_device(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(200 + bits)
    ident = vs.Transform.of()
    for w, h in ((65, 9), (260, 33), (64, 8)):
        src = _noise(rng, 2, w, h, dtype, maxv)
        src[1] = src[1] // 3 + maxv // 4                             # (e): extremes that are not the format's
        for tup in MOTIONS[:3]:
            t = vs.Transform.of(*tup)
            for kw in (dict(), dict(src_stride=3 * w + 1, dst_stride=3 * w + 3)):
                run = lambda f, live, tr, rho: vs.rolling_batch(src, [[f, live]], [[ident, tr]], params=vs.rolling_params(readout=rho), fmt=code, **kw)[0]
                assert np.array_equal(run(0, -1, t, 0.7), src[0])                    # (a) no motion
                assert np.array_equal(run(0, 0, t, 0.0), src[0])                     # (b) rho == 0
                for rho in (-1.0, 0.5, 1.0):
                    assert np.array_equal(run(0, 0, ident, rho), src[0])             # (c) a motion of {0, 0, 0, 0}
                    for f in (0, 1):
                        out = run(f, 0, t, rho)
                        if h % 2 == 1:                                               # (d) the middle row
                            assert np.array_equal(out[(h - 1) // 2], src[f][(h - 1) // 2]), (w, h, tup, rho)
                        for c in range(3):                                           # (e) between the frame's extremes
                            assert src[f][..., c].min() <= out[..., c].min() and out[..., c].max() <= src[f][..., c].max()
                        assert (out != src[f]).mean() > 0.3
    # NULL parameters are the default readout, 0.5
    assert vs.rolling_params().readout == 0.5
    t = vs.Transform.of(*MOTIONS[1])
    src = _noise(rng, 1, 65, 9, dtype, maxv)
    assert np.array_equal(vs.rolling_batch(src, [[0, 0]], [[ident, t]], fmt=code), _want(vs, src, [[0, 0]], [[ident, t]], 0.5, maxv))


def test_device_memory_equals_host_memory(gpu_vs):
    """device-resident frames, enqueue only: dense; then source and destination one element into their buffers (off a dword: the one-pixel
    form for a width that otherwise takes four pixels per lane), pitched"""
    import torch
    vs = gpu_vs
    rng = np.random.default_rng(5)
    w, h, n_src, n_out = 260, 33, 3, 40
    src = _noise(rng, n_src, w, h, np.uint8, 255)
    cf = np.stack([rng.integers(0, n_src, n_out), np.where(rng.random(n_out) < 0.2, -1, 0)], axis=1).astype(np.int32)
    ct = [[vs.Transform.of(), vs.Transform.of(rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-6, 6), rng.uniform(-6, 6))] for _ in range(n_out)]
    p = vs.rolling_params(readout=0.8)
    want = _want(vs, src, cf, ct, 0.8, 255)
    assert (cf[:, 1] < 0).any() and (cf[:, 1] >= 0).any()
    assert np.array_equal(vs.rolling_batch(src, cf, ct, params=p), want)
    dsrc = torch.from_numpy(src).cuda()
    dout = torch.zeros((n_out, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vs.rolling_batch_device(dsrc.data_ptr(), h * w * 3, n_src, w, h, w * 3, vs.FMT_BGR8, cf, ct, dout.data_ptr(), h * w * 3, w * 3, params=p)
    torch.cuda.synchronize()
    assert np.array_equal(dout.cpu().numpy(), want)
    ss, ds = 3 * w + 7, 3 * w + 5
    host = np.zeros(n_src * h * ss + 8, np.uint8)
    host[1:1 + n_src * h * ss].reshape(n_src, h, ss)[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
    dsrc = torch.from_numpy(host).cuda()
    dout = torch.full((n_out * h * ds + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vs.rolling_batch_device(dsrc.data_ptr() + 1, h * ss, n_src, w, h, ss, vs.FMT_BGR8, cf, ct, dout.data_ptr() + 1, h * ds, ds, params=p)
    torch.cuda.synchronize()
    back = dout.cpu().numpy()
    rows = back[1:1 + n_out * h * ds].reshape(n_out, h, ds)
    assert np.array_equal(rows[:, :, :3 * w].reshape(n_out, h, w, 3), want)
    assert back[0] == 0x5A and (back[1 + n_out * h * ds:] == 0x5A).all() and (rows[:, :, 3 * w:] == 0x5A).all()


def test_argument_errors_and_the_handle_s_setter(gpu_vs):
    vs = gpu_vs
    src = np.zeros((3, 32, 48, 3), np.uint8)
    t = vs.Transform.of(0, 0, 3, 2)
    assert vs.rolling_batch(src, [[0, 1]], [[t, t]]).shape == (1, 32, 48, 3)
    with pytest.raises(vs.VsError, match="error -1"):               # a frame index >= n_src
        vs.rolling_batch(src, [[3, 0]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # entry 0 is the frame itself: it cannot be missing
        vs.rolling_batch(src, [[-1, 1]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # a gray format
        vs.rolling_batch(src, [[0, 1]], [[t, t]], fmt=vs.FMT_GRAY8)
    s = vs.Stabilizer(device=0, lag=4)
    assert s.get_rolling_shutter() == 0.0
    for rho, ok in ((-1.0, True), (1.0, True), (0.25, True), (1.0000001, False), (-1.5, False), (float("nan"), False), (float("inf"), False)):
        if ok:
            s.set_rolling_shutter(rho)
            assert s.get_rolling_shutter() == rho
            assert vs.rolling_batch(src, [[0, 1]], [[t, t]], params=vs.rolling_params(readout=rho)).shape == (1, 32, 48, 3)
        else:
            with pytest.raises(vs.VsError, match="error -1"):
                s.set_rolling_shutter(rho)
            with pytest.raises(vs.VsError, match="error -1"):
                vs.rolling_batch(src, [[0, 1]], [[t, t]], params=vs.rolling_params(readout=rho))
            assert s.get_rolling_shutter() == 0.25
    s.set_rolling_shutter(None)                                      # NULL: off
    assert s.get_rolling_shutter() == 0.0
    assert vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2, rolling_shutter=0.5).get_rolling_shutter() == 0.5        # every warp mode
    big = np.zeros((1, 1, 32768, 3), np.uint8)
    with pytest.raises(vs.VsError, match="error -3: rolling shutter: frames up to 32767 x 32767"):      # VS_ERR_UNSUPPORTED beyond 32767 a side
        vs.rolling_batch(big, [[0, 0]], [[t, t]])


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
W, H = 160, 128
_clips = {}


def _clip():
    """18 frames with translation and rotation jitter and noise of 2 levels, and two frames in the middle that jump 40 px sideways and back:
    the alignment fails going in and coming out"""
    if "c" not in _clips:
        from video_stabilizer_amd import synth
        a = DN.noisy_clip(synth, W, H, 16, 11, 2.0, jitter_b=0.02)[0]
        _clips["c"] = np.concatenate([a[:8], np.roll(a[8:10], 40, axis=2), a[8:]])
    return _clips["c"]


ENGINE = {"alone": (dict(lag=4, crop_pixels=8), dict()),
          "all": (dict(lag=4, crop_pixels=0), dict(deblur=3, denoise=3, border_fill=4, inpaint=1))}


@pytest.mark.parametrize("case", sorted(ENGINE))
def test_the_engine_equals_the_engine_model(gpu_vs, oracle, case):
    vs, O = gpu_vs, oracle
    frames = _clip()
    params, passes = ENGINE[case]
    rho = 0.8
    want = EM.engine_model(O, frames, cvinv=HM.cvinv(vs), deblur=passes.get("deblur", 0), denoise=passes.get("denoise", 0), rolling=rho,
                           fill=passes.get("border_fill", 0), inpaint=IP.inpaint if passes.get("inpaint") else None, **params).outs
    got = frame_by_frame(vs.Stabilizer(device=0, rolling_shutter=rho, **passes, **params), frames)
    off = frame_by_frame(vs.Stabilizer(device=0, **passes, **params), frames)
    assert sorted(got) == sorted(want) == sorted(off) and len(want) > 8
    assert sum(int((got[k] != off[k]).sum()) for k in got) > 0.2 * sum(got[k].size for k in got)      # the pass did something
    same = [k for k in got if np.array_equal(got[k], off[k])]
    assert same, "no frame went through uncorrected: the jump no longer makes an alignment fail"
    for k in sorted(want):
        print(case, k, int((got[k] != want[k]).sum()), "of", got[k].size, "samples differ")
    for k in sorted(want):
        assert np.array_equal(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    # one call, and device memory
    import torch
    out, has = vs.Stabilizer(device=0, rolling_shutter=rho, **passes, **params).process_batch(frames)
    for i, hh in enumerate(has):
        if hh:
            assert np.array_equal(out[i], got[i - 4]), i
    crop = params["crop_pixels"]
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((len(frames), H - 2 * crop, W - 2 * crop, 3), dtype=torch.uint8, device="cuda")
    r, hs = vs.Stabilizer(device=0, rolling_shutter=rho, **passes, **params).process_batch_device(dev.data_ptr(), len(frames), W, H, vs.FMT_BGR8, dout.data_ptr())
    torch.cuda.synchronize()
    res = dout.cpu().numpy()
    assert r == len(got)
    for i, hh in enumerate(hs):
        if hh:
            assert np.array_equal(res[i], got[i - 4]), i


def test_lag_0_and_a_failed_alignment_give_the_uncorrected_frame(gpu_vs):
    vs = gpu_vs
    frames = _clip()
    kw = dict(device=0, crop_pixels=8)
    on = frame_by_frame(vs.Stabilizer(lag=0, rolling_shutter=0.8, **kw), frames)
    off = frame_by_frame(vs.Stabilizer(lag=0, **kw), frames)
    assert sorted(on) == sorted(off) and len(on) > 8
    assert all(np.array_equal(on[k], off[k]) for k in on)
    # lag 4: frame k passes uncorrected exactly where the alignment of frame k + 1 failed
    st, states = vs.Stabilizer(lag=4, rolling_shutter=0.8, **kw), []
    on = {}
    for i, f in enumerate(frames):
        o = st.process(f)
        states.append(st.state()[2])
        if o is not None:
            on[i - 4] = o
    off = frame_by_frame(vs.Stabilizer(lag=4, **kw), frames)
    failed = [k for k in on if not states[k + 1]]
    assert failed and len(failed) < len(on)
    for k in on:
        assert np.array_equal(on[k], off[k]) == (k in failed), k


def test_off_is_the_plain_stabilizer_and_allocates_nothing(gpu_vs):
    """the setter never called, set to off (NULL; readout 0), and on then off again: the same bytes as a handle that never heard of the pass,
    and not one allocation more; on: exactly one more (the pass's scratch)"""
    vs = gpu_vs
    frames = _clip()
    kw = dict(device=0, lag=4, crop_pixels=8)

    def run(setup):
        s = vs.Stabilizer(**kw)
        setup(s)
        vs.test_fail_alloc(1 << 30)
        out, has = s.process_batch(frames)
        return vs.test_fail_alloc(0), has, out
    run(lambda s: None)                                              # (the process-wide staging pool fills on the first call)
    n0, has0, out0 = run(lambda s: None)
    for setup in (lambda s: s.set_rolling_shutter(None), lambda s: s.set_rolling_shutter(0.0),
                  lambda s: (s.set_rolling_shutter(0.6), s.set_rolling_shutter(0.0))):
        n, has, out = run(setup)
        assert has == has0 and np.array_equal(out, out0) and n == n0
    n, has, out = run(lambda s: s.set_rolling_shutter(0.6))
    assert has == has0 and not np.array_equal(out, out0) and n == n0 + 1
    # switched on in mid-sequence: takes effect with the next output frame and equals a handle that had it from the start
    a, b, c = vs.Stabilizer(**kw), vs.Stabilizer(**kw), vs.Stabilizer(rolling_shutter=0.6, **kw)
    for i, f in enumerate(frames):
        if i == 6:
            a.set_rolling_shutter(0.6)
        if i == 12:
            a.set_rolling_shutter(None)
        oa, ob, oc = a.process(f), b.process(f), c.process(f)
        if oa is not None:
            assert np.array_equal(oa, oc if 6 <= i < 12 else ob), i


def test_direction_through_the_c_abi(gpu_vs):
    vs = gpu_vs
    ident = vs.Transform.of()

    def correct(frame, tr, rho):
        return vs.rolling_batch(frame[None], [[0, 0]], [[ident, vs.Transform.of(*tr)]], params=vs.rolling_params(readout=rho))[0]
    errs = direction_errors(correct)
    for raw, right, wrong in errs:
        print("raw %.3f  corrected %.3f (%.2f)  rho negated %.3f (%.2f)" % (raw, right, right / raw, wrong, wrong / raw))
    for raw, right, wrong in errs:
        assert right < 0.5 * raw
        assert wrong > raw
