"""The lens map and the remap on the GPU (include/vs_amd.h: vs_lens_map, vs_bgr_remap_batch) against the rule's restatement
(tests/_lens_ref.py).  np.array_equal throughout: the rules fix every bit.  The direction test through the C ABI."""
import numpy as np
import pytest

import _lens_ref as L
from test_lens_cpu import COEFFS

pytestmark = pytest.mark.gpu

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr16": (4, np.uint16, 16)}
# below a row's eight-element load (1 x 1, 2 x 2); a frame smaller than a wave; strip and row-group seams; the 256-column seam of the
# four-pixel form; a width that refuses that form
SHAPES = [(1, 1), (2, 2), (7, 5), (64, 8), (65, 9), (260, 32), (258, 16)]


def _noise(rng, n, w, h, dtype, maxv):
    return rng.integers(0, maxv + 1, (n, h, w, 3)).astype(dtype)


def _map(rng, w, h, ow, oh):
    """positions from three pixels outside the w x h frame on every side, all fractions; a smooth part (neighbours read neighbours) in the
    upper half, noise in the lower"""
    u, v = np.meshgrid(np.arange(ow), np.arange(oh))
    smooth = np.stack([(u * (w + 5.0) / ow - 2.5) * 32 + 7 * v, (v * (h + 5.0) / oh - 2.5) * 32 - 3 * u], axis=2).astype(np.int64)
    noise = np.stack([rng.integers(-96, 32 * w + 96, (oh, ow)), rng.integers(-96, 32 * h + 96, (oh, ow))], axis=2)
    return np.where((v < (oh + 1) // 2)[..., None], smooth, noise).astype(np.int32)


def test_the_device_map_equals_the_host_map(gpu_vs):
    import torch
    vs = gpu_vs
    for name in sorted(COEFFS):
        for w, h, ms in ((1, 1, 2), (2, 3, 9), (96, 64, 2 * 96), (65, 5, 2 * 65 + 3), (1920, 8, 2 * 1920 + 6)):
            p = vs.lens_params(w, h, **COEFFS[name])
            want = vs.lens_map(p, w, h)
            assert np.array_equal(want, L.lens_map(L.params(w, h, **COEFFS[name]), w, h))
            dev = torch.full(((h + 4) * ms,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            vs.lens_map_device(p, w, h, dev.data_ptr() + 2 * ms * 4, ms)
            torch.cuda.synchronize()
            back = dev.cpu().numpy().reshape(h + 4, ms)
            assert np.array_equal(back[2:h + 2, :2 * w].reshape(h, w, 2), want), (name, w, h)
            assert (back[:2] == 0x5A5A5A5A).all() and (back[h + 2:] == 0x5A5A5A5A).all() and (back[2:h + 2, 2 * w:] == 0x5A5A5A5A).all()


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_remap_batch_equals_the_rule(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(300 + bits)
    guard = 0x5A if bits == 8 else 0x5A5A
    interpolated = 0
    for w, h in SHAPES:
        src = _noise(rng, 3, w, h, dtype, maxv)
        pos = _map(rng, w, h, w, h)
        interpolated += int(((pos & 31) != 0).any(axis=2).sum())
        for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
            want = L.remap_batch(src, pos, border, maxv)
            got = vs.remap_batch(src, pos, border=border, fmt=code)
            assert np.array_equal(got, want), (w, h, border, int((got != want).sum()))
            # pitched rows on all three sides: odd (the destination's rows leave the dwords: the one-pixel form), then rows that start on
            # dwords; the destination's padding must stay untouched
            for ss, ds, ms in ((3 * w + 7, 3 * w + 5, 2 * w + 3), (3 * w + 8, 3 * w + 4, 2 * w + 4)):
                res, padded = vs.remap_batch(src, pos, border=border, fmt=code, src_stride=ss, dst_stride=ds, map_stride=ms, guard=guard)
                assert np.array_equal(res, want), (w, h, border, ss, ds)
                assert (padded[:, :, 3 * w:] == guard).all()
    assert interpolated > 10000


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_output_sizes_other_than_the_frame_s(gpu_vs, fmt):
    """ow x oh larger and smaller than w x h, across the forms: a wide source with a tiny map, a source below the eight-element load with a
    map that takes four pixels per lane"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(400 + bits)
    for (w, h), (ow, oh) in (((65, 9), (260, 33)), ((260, 32), (7, 5)), ((2, 2), (64, 8)), ((7, 5), (1, 1)), ((64, 8), (65, 9))):
        src = _noise(rng, 2, w, h, dtype, maxv)
        pos = _map(rng, w, h, ow, oh)
        for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
            got = vs.remap_batch(src, pos, border=border, fmt=code)
            assert got.shape == (2, oh, ow, 3)
            assert np.array_equal(got, L.remap_batch(src, pos, border, maxv)), (w, h, ow, oh, border)


@pytest.mark.parametrize("shape", [(65, 9), (64, 8)])
def test_frame_counts_around_the_slice(gpu_vs, shape):
    """n = 1, slice - 1, slice, slice + 1, 2 slice + 1: a workgroup takes a pixel through a slice of the call's frames"""
    vs = gpu_vs
    w, h = shape
    s = vs.REMAP_SLICE
    rng = np.random.default_rng(17)
    src = _noise(rng, 2 * s + 1, w, h, np.uint8, 255)
    pos = _map(rng, w, h, w, h)
    want = L.remap_batch(src, pos, vs.BORDER_CLAMP, 255)
    assert len({want[i].tobytes() for i in range(len(want))}) == len(want)       # every frame's output is its own
    for n in (1, s - 1, s, s + 1, 2 * s + 1):
        assert np.array_equal(vs.remap_batch(src[:n], pos), want[:n]), n


def test_the_rule_s_consequences_on_the_device(gpu_vs):
    vs = gpu_vs
    rng = np.random.default_rng(23)
    for fmt in sorted(FORMATS):
        code, dtype, bits = FORMATS[fmt]
        maxv = (1 << bits) - 1
        for w, h in ((65, 9), (260, 32), (2, 2)):
            src = _noise(rng, 2, w, h, dtype, maxv)
            src[1] = src[1] // 3 + maxv // 4
            u, v = np.meshgrid(np.arange(w), np.arange(h))
            ident = np.stack([32 * u, 32 * v], axis=2)
            for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):     # (a)
                assert np.array_equal(vs.remap_batch(src, ident, border=border, fmt=code), src)
            out = vs.remap_batch(src, _map(rng, w, h, w, h), fmt=code)                 # (b)
            for f in range(2):
                for c in range(3):
                    assert src[f][..., c].min() <= out[f][..., c].min() and out[f][..., c].max() <= src[f][..., c].max()
    # (a) through the lens: the identity lens's map returns every frame
    w, h = 96, 64
    src = _noise(rng, 2, w, h, np.uint8, 255)
    assert np.array_equal(vs.remap_batch(src, vs.lens_map(vs.lens_params(w, h), w, h)), src)


def test_device_memory_equals_host_memory(gpu_vs):
    """device-resident frames and map, enqueue only: dense; then source, map and destination one element into their buffers (the
    destination off a dword: the one-pixel form for a width that otherwise takes four pixels per lane), pitched, with guards"""
    import torch
    vs = gpu_vs
    rng = np.random.default_rng(5)
    w, h, ow, oh, n = 260, 33, 256, 40, 11
    src = _noise(rng, n, w, h, np.uint8, 255)
    pos = _map(rng, w, h, ow, oh)
    for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
        want = L.remap_batch(src, pos, border, 255)
        assert np.array_equal(vs.remap_batch(src, pos, border=border), want)
        dsrc, dmap = torch.from_numpy(src).cuda(), torch.from_numpy(pos).cuda()
        dout = torch.zeros((n, oh, ow, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vs.remap_batch_device(dsrc.data_ptr(), h * w * 3, n, w, h, w * 3, vs.FMT_BGR8, dmap.data_ptr(), 2 * ow, ow, oh, dout.data_ptr(), oh * ow * 3, ow * 3,
                              border=border)
        torch.cuda.synchronize()
        assert np.array_equal(dout.cpu().numpy(), want)
        ss, ds, ms = 3 * w + 7, 3 * ow + 5, 2 * ow + 3
        host = np.zeros(n * h * ss + 8, np.uint8)
        host[1:1 + n * h * ss].reshape(n, h, ss)[:, :, :3 * w] = src.reshape(n, h, 3 * w)
        hmap = np.full(oh * ms + 2, 0x5A5A5A5A, np.int32)
        hmap[1:1 + oh * ms].reshape(oh, ms)[:, :2 * ow] = pos.reshape(oh, 2 * ow)
        dsrc, dmap = torch.from_numpy(host).cuda(), torch.from_numpy(hmap).cuda()
        dout = torch.full((n * oh * ds + 8,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vs.remap_batch_device(dsrc.data_ptr() + 1, h * ss, n, w, h, ss, vs.FMT_BGR8, dmap.data_ptr() + 4, ms, ow, oh, dout.data_ptr() + 1, oh * ds, ds, border=border)
        torch.cuda.synchronize()
        back = dout.cpu().numpy()
        rows = back[1:1 + n * oh * ds].reshape(n, oh, ds)
        assert np.array_equal(rows[:, :, :3 * ow].reshape(n, oh, ow, 3), want)
        assert back[0] == 0x5A and (back[1 + n * oh * ds:] == 0x5A).all() and (rows[:, :, 3 * ow:] == 0x5A).all()


def test_the_remap_s_argument_errors(gpu_vs):
    vs = gpu_vs
    src = np.zeros((2, 6, 8, 3), np.uint8)
    pos = np.zeros((4, 5, 2), np.int32)
    assert vs.remap_batch(src, pos).shape == (2, 4, 5, 3)
    with pytest.raises(vs.VsError, match="error -1"):               # a gray format
        vs.remap_batch(src, pos, fmt=vs.FMT_GRAY8)
    with pytest.raises(vs.VsError, match="error -1"):               # no such border
        vs.remap_batch(src, pos, border=2)
    out = np.zeros((2, 4, 5, 3), np.uint8)

    def raw(n=2, ss=24, ms=10, ds=15, s=src, m=pos, o=out):
        return vs.lib().vs_bgr_remap_batch(vs._p(s) if s is not None else None, 6 * 24, n, 8, 6, ss, vs.FMT_BGR8, vs._p(m) if m is not None else None, ms, 5, 4,
                                           vs.BORDER_CLAMP, vs._p(o) if o is not None else None, 4 * 15, ds, vs.MEM_HOST, None)
    assert raw() == 0
    # rows that do not hold their pixels or pairs, no frames, null pointers
    for kw in (dict(ms=9), dict(ds=14), dict(ss=23), dict(n=0), dict(s=None), dict(m=None), dict(o=None)):
        assert raw(**kw) == -1, kw
    with pytest.raises(vs.VsError, match="error -3: remap: frames and maps up to 32767 x 32767"):       # VS_ERR_UNSUPPORTED beyond 32767 a side
        vs.remap_batch(np.zeros((1, 1, 32768, 3), np.uint8), pos)
    with pytest.raises(vs.VsError, match="error -3: remap: frames and maps up to 32767 x 32767"):
        vs.remap_batch(src[:1], np.zeros((1, 32768, 2), np.int32))


def test_direction_through_the_c_abi(gpu_vs):
    vs = gpu_vs

    def correct(frame, p):
        h, w, _ = frame.shape
        return vs.remap_batch(frame[None], vs.lens_map(vs.lens_params(w, h, **{k: float(v) for k, v in p.items()}), w, h))[0]
    errs = L.direction_errors(correct)
    for raw, right, wrong in errs:
        print("raw %.3f  corrected %.3f (%.3f)  negated %.3f (%.2f)" % (raw, right, right / raw, wrong, wrong / raw))
    for raw, right, wrong in errs:
        assert right <= 0.1 * raw
        assert wrong >= 1.1 * raw


# ---- engine level -----------------------------------------------------------------------------------------------------------------------
# The definition: a handle with the correction on, fed raw frames, returns bit for bit what a handle with it off returns when fed
# vs_bgr_remap_batch(raw, vs_lens_map(params)) -- outputs, has_output and vs_stabilizer_state.
W, H, LAG = 96, 64, 4
LENS = dict(k1=-0.2, k2=0.05, p1=0.001, p2=-0.002, zoom=1.05)
PYR = dict(pyramid_min_width=10, pyramid_min_height=10)             # (96 x 64 has two levels above 20 x 20; the aligner wants three)
ENGINE = {"alone": (dict(lag=LAG, crop_pixels=8, **PYR), dict()),
          "all": (dict(lag=LAG, crop_pixels=0, **PYR), dict(deblur=3, denoise=3, rolling_shutter=0.6, border_fill=4, inpaint=1))}
_clips = {}


def _clip(n):
    """n frames with translation and rotation jitter; in the longer clips two frames jump 30 px sideways and back: alignments fail"""
    if n not in _clips:
        from video_stabilizer_amd import synth
        a = synth.make_clip(W, H, n, seed=11, channels=3)[0]
        if n >= 16:
            a = np.concatenate([a[:8], np.roll(a[8:10], 30, axis=2), a[10:]])
        _clips[n] = np.ascontiguousarray(a)
    return _clips[n]


def _state(st):
    m, a, ok = st.state()
    return m.tup(), a.tup(), ok


def _run(vs, frames, how, lens, border, params, passes, n_clips=0):
    """-> (outputs (n, oh, ow, 3), has_output, state).  lens: the correction is on in the handle; else the handle never hears of it"""
    import torch
    kw = dict(lens=(vs.lens_params(W, H, border=border, **LENS), W, H)) if lens else dict()
    st = vs.Stabilizer(device=0, **kw, **passes, **params)
    assert (st.get_lens() is not None) == bool(lens)
    n, crop = len(frames), params["crop_pixels"]
    if how == "single":
        out, has = np.zeros((n, H - 2 * crop, W - 2 * crop, 3), np.uint8), []
        for i, f in enumerate(frames):
            o = st.process(f)
            has.append(int(o is not None))
            if o is not None:
                out[i] = o
    elif how == "batch":
        out, has = st.process_batch(frames)
    elif how == "clips":
        out, has = st.process_clips(frames, n_clips)
    else:
        dev = torch.from_numpy(frames).cuda()
        dout = torch.zeros((n, H - 2 * crop, W - 2 * crop, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if how == "device":
            _, has = st.process_batch_device(dev.data_ptr(), n, W, H, vs.FMT_BGR8, dout.data_ptr())
        else:
            _, has = st.process_clips_device(dev.data_ptr(), n_clips, n // n_clips, W, H, vs.FMT_BGR8, dout.data_ptr())
        torch.cuda.synchronize()
        out = dout.cpu().numpy()
    return out, list(has), _state(st)


def _corrected(vs, frames, border):
    return vs.remap_batch(frames, vs.lens_map(vs.lens_params(W, H, **LENS), W, H), border=border)


def _same(a, b, what):
    assert a[1] == b[1], what
    assert a[2] == b[2], what
    assert np.array_equal(a[0], b[0]), (what, int((a[0] != b[0]).sum()))


@pytest.mark.parametrize("case", sorted(ENGINE))
def test_the_engine_with_the_correction_on_equals_the_engine_fed_corrected_frames(gpu_vs, case):
    vs = gpu_vs
    params, passes = ENGINE[case]
    raw = _clip(18)
    for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
        fixed = _corrected(vs, raw, border)
        assert (fixed != raw).mean() > 0.05                          # (the synthetic scene is flat between its edges)
        want = _run(vs, fixed, "batch", False, border, params, passes)
        plain = _run(vs, raw, "batch", False, border, params, passes)
        assert sum(want[1]) == len(raw) - LAG and not np.array_equal(want[0], plain[0])
        for how in ("batch", "single", "device"):
            _same(_run(vs, raw, how, True, border, params, passes), want, (case, border, how))
        if border == vs.BORDER_CONSTANT:
            break                                                    # (the other routes below: under the clamp border only)
        # a clip batch: three clips of six frames, host and device memory
        wantc = _run(vs, fixed, "clips", False, border, params, passes, n_clips=3)
        assert sum(wantc[1]) == 3 * (6 - LAG)
        for how in ("clips", "clips_device"):
            _same(_run(vs, raw, how, True, border, params, passes, n_clips=3), wantc, (case, how))


_CHILD = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
torch.cuda.init()
import numpy as np
from video_stabilizer_amd import capi as vs
import test_lens_gpu as T
params, passes = T.ENGINE["alone"]
raw = T._clip(96)
fixed = T._corrected(vs, raw, vs.BORDER_CLAMP)
# one device-dense batch long enough for the time-chunk route (n >= 96), and a clip batch long enough for the group route
T._same(T._run(vs, raw, "device", True, vs.BORDER_CLAMP, params, passes), T._run(vs, fixed, "device", False, vs.BORDER_CLAMP, params, passes), "long clip")
T._same(T._run(vs, raw, "clips_device", True, vs.BORDER_CLAMP, params, passes, n_clips=8),
        T._run(vs, fixed, "clips_device", False, vs.BORDER_CLAMP, params, passes, n_clips=8), "clip batch")
T._same(T._run(vs, raw, "device", True, vs.BORDER_CLAMP, params, passes), T._run(vs, fixed, "batch", False, vs.BORDER_CLAMP, params, passes), "device against host")
print("routes ok")
"""


@pytest.mark.parametrize("overlap", ["0", "1"])
def test_the_long_routes_with_and_without_the_overlap(gpu_vs, overlap):
    """VS_STAB_OVERLAP is read once per process: a child each.  With the correction on a dense device batch takes the plain route; the handle
    fed corrected frames takes the overlapped one (VS_STAB_OVERLAP=1): the same bytes either way"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VS_STAB_OVERLAP=overlap)
    out = subprocess.run([sys.executable, "-c", _CHILD % (root, os.path.join(root, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "routes ok" in out.stdout


def test_off_is_the_plain_stabilizer_and_allocates_nothing(gpu_vs):
    """never set, set to NULL, set to the identity lens, on then off: the same bytes as a handle that never heard of the pass and not one
    allocation more; on: more allocations (the map, the corrected batch) and other bytes"""
    vs = gpu_vs
    frames = _clip(18)
    kw = dict(device=0, lag=LAG, crop_pixels=8, **PYR)
    lens = vs.lens_params(W, H, **LENS)

    def run(setup):
        s = vs.Stabilizer(**kw)
        setup(s)
        vs.test_fail_alloc(1 << 30)
        out, has = s.process_batch(frames)
        return vs.test_fail_alloc(0), has, out, _state(s)
    run(lambda s: None)                                              # (the process-wide staging pool fills on the first call)
    n0, has0, out0, st0 = run(lambda s: None)
    for setup in (lambda s: s.set_lens(None), lambda s: s.set_lens(vs.lens_params(W, H), W, H), lambda s: s.set_lens(vs.lens_params(W, H, fx=50.0, cx=3.0), W, H),
                  lambda s: (s.set_lens(lens, W, H), s.set_lens(None))):
        n, has, out, st = run(setup)
        assert has == has0 and np.array_equal(out, out0) and st == st0 and n == n0
    n, has, out, st = run(lambda s: s.set_lens(lens, W, H))
    assert has == has0 and not np.array_equal(out, out0) and n > n0


def test_the_setter_s_errors_and_frames_of_another_size(gpu_vs):
    vs = gpu_vs
    s = vs.Stabilizer(device=0, lag=LAG, crop_pixels=8, **PYR)
    assert s.get_lens() is None
    lens = vs.lens_params(W, H, **LENS)
    s.set_lens(lens, W, H)
    p, w, h = s.get_lens()
    assert p.tup() == lens.tup() and (w, h) == (W, H)
    for kw in (dict(k1=float("nan")), dict(fx=0.0), dict(zoom=-1.0), dict(cy=float("inf")), dict(border=2)):
        with pytest.raises(vs.VsError, match="error -1"):
            s.set_lens(vs.lens_params(W, H, **dict(LENS, **kw)), W, H)
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_lens(lens, 0, H)
    with pytest.raises(vs.VsError, match="error -3"):
        s.set_lens(lens, 32768, H)
    assert s.get_lens()[0].tup() == lens.tup()                       # a refused call leaves the setting
    # a frame of another size while the pass is on: VS_ERR_ARG before any work -- the sequence goes on as if the call had not been made
    frames = _clip(18)
    ref = vs.Stabilizer(device=0, lag=LAG, crop_pixels=8, lens=(lens, W, H), **PYR)
    for i, f in enumerate(frames):
        if i == 9:
            with pytest.raises(vs.VsError, match="error -1.*lens correction is set for 96 x 64"):
                s.process(np.zeros((H + 2, W, 3), np.uint8))
            with pytest.raises(vs.VsError, match="error -1"):
                s.process_batch(np.zeros((3, H, W - 4, 3), np.uint8))
        a, b = s.process(f), ref.process(f)
        assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), i
        assert _state(s) == _state(ref)
    s.set_lens(None)                                                 # off: any size again
    assert s.get_lens() is None
    s.process(np.zeros((H + 2, W, 3), np.uint8))


def test_video_test_with_a_lens_writes_what_the_corrected_stabilizer_returns(gpu_vs, tmp_path):
    """apps/vs_video_test --lens fx,fy,cx,cy,k1,k2,p1,p2,k3 --lens-zoom z: the file holds what a handle with that lens returns"""
    import os
    import subprocess
    vs = gpu_vs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "apps"), "-s", "-j4"])
    from video_stabilizer_amd import synth
    w, h = 160, 128                                                  # (the program runs the default aligner parameters: three levels above 20 x 20)
    frames = synth.make_clip(w, h, 18, seed=11, channels=3)[0]
    (tmp_path / "in").mkdir()
    frames.tofile(tmp_path / "in" / ("clip_%dx%d.bgr" % (w, h)))
    r = subprocess.run([os.path.join(root, "apps", "bin", "vs_video_test"), str(tmp_path / "in"), str(tmp_path / "out"), "--crop", "8", "--chunk", "7",
                        "--lens", "150.5,151,79,63.25,-0.2,0.05,0.001,-0.002,0.01", "--lens-zoom", "1.05"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lens = vs.lens_params(w, h, fx=150.5, fy=151.0, cx=79.0, cy=63.25, k1=-0.2, k2=0.05, p1=0.001, p2=-0.002, k3=0.01, zoom=1.05)
    on, off = vs.Stabilizer(device=0, crop_pixels=8, lens=(lens, w, h)), vs.Stabilizer(device=0, crop_pixels=8)
    want = np.stack([o for o in (on.process(f) for f in frames) if o is not None])
    plain = np.stack([o for o in (off.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_clip_%dx%d.bgr" % (w, h)), np.uint8).reshape(-1, h - 16, w - 16, 3)
    assert np.array_equal(got, want) and not np.array_equal(want, plain)
    r = subprocess.run([os.path.join(root, "apps", "bin", "vs_video_test"), str(tmp_path / "in"), str(tmp_path / "out"), "--lens", "90,90,47,31"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--lens takes" in r.stderr
