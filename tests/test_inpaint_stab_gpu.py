"""The stabilizer's inpaint (include/vs_amd.h: vs_stabilizer_set_inpaint) on the GPU: every route gives the same bytes; on and off differ only
where the model says nothing covers; the inpaint-on output IS the rule applied to the inpaint-off output under the model's still-open mask
(tests/_inpaint_ref.py on tests/_engine_model.py's masks); the default crop pays nothing; the deflicker's gain stays last; allocation
failures and poisoned fresh allocations.  Frames without zero samples throughout, so that a black border cannot coincide with a sample."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _engine_model as EM
import _inpaint_ref as R
from _stab_routes import assert_every_route_equals, frame_by_frame, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240


def _clip(n, seed, bits=8, w=W, h=H, **kw):
    from video_stabilizer_amd import synth
    return np.maximum(synth.make_clip(w, h, n, seed=seed, channels=3, bits=bits, **kw)[0], 1)


def _cut_clip(bits):
    """33 frames with a three-frame scene cut in the middle: the alignment fails there and the candidate lists end early"""
    a = _clip(30, 5, bits)
    return np.concatenate([a[:14], _clip(3, 77, bits), a[14:]])


@pytest.mark.parametrize("bits", [8, 10])
def test_every_route_gives_the_same_frames(gpu_vs, bits):
    """process frame by frame == process_batch (one call; split calls) == device memory == process_clips (host, device), inpaint on"""
    import torch
    vs = gpu_vs
    frames = _cut_clip(bits)
    n = len(frames)
    kw = dict(device=0, lag=6, crop_pixels=0, border_fill=4, inpaint=1)
    ref = frame_by_frame(vs.Stabilizer(**kw), frames)
    plain = frame_by_frame(vs.Stabilizer(**dict(kw, inpaint=0)), frames)
    assert any(not np.array_equal(ref[k], plain[k]) for k in ref)    # the pass did something
    assert_every_route_equals(vs, kw, frames, ref, (3, 1, 9, 2, 11, n - 26))
    fmt = vs.FMT_BGR8 if bits == 8 else vs.FMT_BGR10
    # two clips of 16 frames through process_clips: each equals the clip on a handle of its own
    fpc = 16
    two = np.ascontiguousarray(frames[:2 * fpc])
    refs = [frame_by_frame(vs.Stabilizer(**kw), two[:fpc]), frame_by_frame(vs.Stabilizer(**kw), two[fpc:])]
    out, has = vs.Stabilizer(**kw).process_clips(two, 2)
    dtwo = torch.from_numpy(two.view(np.int16) if bits != 8 else two).cuda()
    dout2 = torch.zeros((2 * fpc, H, W, 3), dtype=dtwo.dtype, device="cuda")
    assert dtwo.shape[0] == 2 * fpc
    r, dhas = vs.Stabilizer(**kw).process_clips_device(dtwo.data_ptr(), 2, fpc, W, H, fmt, dout2.data_ptr())
    torch.cuda.synchronize()
    res = dout2.cpu().numpy().view(frames.dtype)
    assert has == dhas and sum(has) == 2 * (fpc - 6)
    for c in range(2):
        for i in range(fpc):
            if has[c * fpc + i]:
                assert np.array_equal(out[c * fpc + i], refs[c][i - 6]) and np.array_equal(res[c * fpc + i], refs[c][i - 6]), (c, i)


def test_time_chunks_and_the_pipelined_host_batch(gpu_vs, monkeypatch):
    """a device-resident clip long enough for the time chunks (warps, coverage and inpaint on the warp stream, the next chunk's alignment
    prefetched) and a host batch long enough for the upload / compute / download pipeline, against calls that stay below both thresholds"""
    import torch
    vs = gpu_vs
    w, h, n = 160, 128, 130
    frames = _clip(n, 9, w=w, h=h, pan=0.2)
    monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(37 * w * h * 3))  # host batches: upload chunks of 37 frames (read at every call)
    kw = dict(device=0, lag=6, crop_pixels=0, border_fill=2, inpaint=1)
    st = vs.Stabilizer(**kw)
    ref = np.zeros_like(frames)
    ref_has = []
    for p in range(0, n, 20):                                        # short calls: one chunk each, no overlap
        o, hs = st.process_batch(frames[p:p + 20])
        ref[p:p + 20] = o
        ref_has += hs
    plain, _ = vs.Stabilizer(**dict(kw, inpaint=0)).process_batch(frames[:20])
    assert not np.array_equal(plain, ref[:20])
    out, has = vs.Stabilizer(**kw).process_batch(frames)            # host memory, one call: pipelined
    assert has == ref_has and np.array_equal(out, ref)
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    r, hs = vs.Stabilizer(**kw).process_batch_device(dev.data_ptr(), n, w, h, vs.FMT_BGR8, dout.data_ptr())     # time chunks
    torch.cuda.synchronize()
    assert hs == ref_has and np.array_equal(dout.cpu().numpy(), ref)


@pytest.mark.parametrize("fill", [4, 0])
@pytest.mark.parametrize("bits", [8, 10])
def test_inpaint_on_is_the_rule_on_the_inpaint_off_output(gpu_vs, oracle, bits, fill):
    """for every frame whose inpaint-off output equals the engine model's (a coverage decision can flip on a 1e-12 transform difference: at
    most one frame may be left out), inpaint on == inpaint_ref(inpaint off, the model's still-open mask), bit for bit; and on and off
    differ only inside that mask"""
    vs, O = gpu_vs, oracle
    frames = _cut_clip(bits)
    kw = dict(lag=6, crop_pixels=0)
    model = EM.engine_model(O, frames, fill=fill, want_masks=True, **kw)
    off = frame_by_frame(vs.Stabilizer(device=0, border_fill=fill, **kw), frames)
    on = frame_by_frame(vs.Stabilizer(device=0, border_fill=fill, inpaint=1, **kw), frames)
    assert sorted(off) == sorted(model.outs) == sorted(on)
    left_out, open_px, changed = [], 0, 0
    for k, want in model.outs.items():
        still_open = model.masks[k][1]
        if not np.array_equal(off[k], want):
            left_out.append(k)
            continue
        # (an open pixel is not always black: with one to three taps inside the frame the constant border is blended in.  The rule never reads it.)
        assert np.array_equal(on[k][~still_open], off[k][~still_open]), k
        assert np.array_equal(on[k], R.inpaint(off[k], ~still_open)), k
        open_px += int(still_open.sum())
        changed += int((on[k] != off[k]).any(-1).sum())
    print("%d-bit fill %d: %d frames, %d left out, %d open pixels, %d changed" % (bits, fill, len(model.outs), len(left_out), open_px, changed))
    assert len(left_out) <= 1, left_out
    assert open_px > 0 and 0.9 * open_px < changed <= open_px        # (no sample is zero: an inpainted pixel differs from a black one)


def test_default_crop_pays_nothing(gpu_vs):
    """default crop and jitter: every frame's own source covers the window, the host test skips the pass -- the same bytes, and not one
    allocation more than with the switch off"""
    vs = gpu_vs
    frames = _clip(24, 7)
    kw = dict(device=0, lag=6, border_fill=3)

    def run(**extra):
        s = vs.Stabilizer(**dict(kw, **extra))
        vs.test_fail_alloc(1 << 30)
        out, has = s.process_batch(frames)
        return vs.test_fail_alloc(0), has, out
    run()                                                            # (the process-wide staging pool fills on the first call)
    n_off, has_off, out_off = run()
    n_on, has_on, out_on = run(inpaint=1)
    assert has_on == has_off and sum(has_on) > 0 and np.array_equal(out_on, out_off)
    assert n_on == n_off
    n_crop0 = run(inpaint=1, crop_pixels=0)[0]
    assert n_crop0 == run(crop_pixels=0)[0] + 1                      # the pass's one scratch block


def test_the_deflickers_gain_stays_last(gpu_vs):
    """with deflicker on the output is gain(inpaint(warp)), not inpaint(gain(warp)).  The gain is a per-frame, per-channel map of sample
    values: read off the covered pixels (inpaint-off output without and with deflicker), it must take the inpaint-only output to the
    output with both on, wherever the value occurs among the covered pixels"""
    vs = gpu_vs
    frames = _clip(30, 5).astype(np.float64)
    frames = np.clip(frames * (0.8 + 0.15 * np.sin(np.arange(30) * 1.3))[:, None, None, None], 1, 255).astype(np.uint8)
    kw = dict(device=0, lag=6, crop_pixels=0, border_fill=2)
    w_ = frame_by_frame(vs.Stabilizer(**kw), frames)                              # warp
    y_ = frame_by_frame(vs.Stabilizer(deflicker=4, **kw), frames)                 # gain(warp)
    z_ = frame_by_frame(vs.Stabilizer(inpaint=1, **kw), frames)                   # inpaint(warp)
    x_ = frame_by_frame(vs.Stabilizer(inpaint=1, deflicker=4, **kw), frames)      # both
    checked = scaled = 0
    for k in w_:
        open_ = (z_[k] != w_[k]).any(-1)
        for c in range(3):
            table = np.full(256, -1, np.int64)
            table[w_[k][..., c][~open_]] = y_[k][..., c][~open_]
            assert np.array_equal(table[w_[k][..., c][~open_]], y_[k][..., c][~open_])         # one map per channel: the premise
            zi = z_[k][..., c][open_]
            known = table[zi] >= 0
            assert np.array_equal(x_[k][..., c][open_][known], table[zi][known]), (k, c)
            checked += int(known.sum())
            scaled += int((table[zi][known] != zi[known]).sum())
        assert np.array_equal(x_[k][~open_], y_[k][~open_])
    assert checked > 1000 and scaled > 0


@pytest.mark.parametrize("throwing", [False, True])
def test_inpainted_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    vs = gpu_vs
    frames = _clip(16, 7, w=160, h=128)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    kw = dict(device=0, lag=4, smoother_memory=2, crop_pixels=0, border_fill=3)

    def allocations(make):
        h = make()
        vs.test_fail_alloc(1 << 30)
        call(h)
        return vs.test_fail_alloc(0)
    allocations(lambda: vs.Stabilizer(**kw))                         # (the process-wide staging pool fills on the first call)
    n_off, n_on = allocations(lambda: vs.Stabilizer(**kw)), allocations(lambda: vs.Stabilizer(inpaint=1, **kw))
    assert n_on == n_off + 1                                         # the scratch block joins the protocol
    fired = walk(vs, lambda: vs.Stabilizer(inpaint=1, **kw), call, n_on, throwing)
    print("inpainted process_batch: %d allocations failed one by one (%s)" % (fired, "throwing" if throwing else "error code"))
    assert fired == n_on


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from video_stabilizer_amd import capi as G, synth
dig = hashlib.sha256()
def put(*xs):
    for x in xs:
        dig.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
rng = np.random.default_rng(5)
for dtype, maxv, fmt, (w, h) in ((np.uint8, 255, G.FMT_BGR8, (300, 270)), (np.uint16, 1023, G.FMT_BGR10, (129, 65)), (np.uint8, 255, G.FMT_BGR8, (9, 1))):
    img = rng.integers(0, maxv + 1, (3, h, w, 3)).astype(dtype)
    mask = (rng.random((3, h, w)) < 0.4).astype(np.uint8)
    mask[1] = 1
    put(G.bgr_inpaint_batch(img, mask, fmt=fmt), G.bgr_inpaint_batch(img, mask, fmt=fmt, stride=3 * w + 7, mask_stride=w + 3))
t = [[G.Transform.of(0.01, -0.02, 7.5, -3.0), G.Transform.of(-0.01, 0.02, -9.0, 4.0)]]
put(G.bgr_fill_coverage_batch(300, 270, [[0, 1]], t), G.bgr_fill_coverage_batch(300, 270, [[0, 1]], t, roi=(3, 5, 257, 129)))
clip = np.maximum(synth.make_clip(160, 128, 20, seed=5, channels=3)[0], 1)
clip = np.concatenate([clip[:9], np.maximum(synth.make_clip(160, 128, 3, seed=77, channels=3)[0], 1), clip[9:]])
for kw in (dict(inpaint=1), dict(inpaint=1, border_fill=3), dict(inpaint=1, border_fill=3, deflicker=2, denoise=2)):
    kw = dict(dict(device=0, lag=5, crop_pixels=0), **kw)
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
        env = dict(os.environ, VS_TEST_POISON_ALLOC=str(byte), VS_TEST_HOOKS="1")
        out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        _digests[byte] = [line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1]
    return _digests[byte]


def test_inpaint_does_not_depend_on_what_fresh_allocations_contain(gpu_vs):
    # one child process per fill byte
    assert _digest(255) == _digest(0)


def test_video_test_inpaint_writes_what_the_library_returns(gpu_vs, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    frames = _clip(40, 77)
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    exe = os.path.join(ROOT, "apps", "bin", "vs_video_test")
    r = subprocess.run([exe, str(d), str(tmp_path / "out"), "--crop", "0", "--fill", "4", "--inpaint", "--chunk", "13"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = gpu_vs.Stabilizer(device=0, crop_pixels=0, border_fill=4, inpaint=1)
    want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_" + raw.name), np.uint8).reshape(-1, H, W, 3)
    assert np.array_equal(got, want)
    assert (got != 0).all()                                          # crop 0 with no black sliver left
    r = subprocess.run([exe, str(d), str(tmp_path / "out2"), "--inpaint", "--lanczos2"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "vs_stabilizer_set_inpaint" in r.stderr
