"""Deflicker on the GPU (include/vs_amd.h: vs_bgr_exposure_stats_batch, vs_exposure_gains_batch, vs_bgr_gain_batch, vs_stabilizer_set_deflicker)
against the rule's restatement (tests/_deflicker_ref.py).  Kernel level: np.array_equal -- the rule fixes every bit.  Engine: every route gives
the same bytes, and those bytes are the deflicker-off output put through the kernel-level calls with candidates composed here from a
capi.Aligner's measurements (the same host algebra, the same doubles).  Every case asserts its premise on the CPU reference before it looks at
the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _engine_model as EM
import _deflicker_ref as R
from _stab_routes import frame_by_frame, walk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 128
UNIT = 32768
FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}
# frames smaller than a wave; the seams of the statistics' 64-column chunks at step 1 (63 / 64 / 65) and of its 256-column tile (257); widths
# that are and are not multiples of the gain pass's pixel groups; more than one workgroup down (17 rows at step 1 is three strips, 516 x 17 three tiles)
SHAPES = [(1, 1), (3, 2), (63, 9), (64, 9), (65, 9), (257, 17), (516, 17)]
STEPS = (1, 4, 64)
KINDS = ("noise", "constant", "black", "clipped")


def _o(O, t):
    return O.Transform.of(*t.tup())


def _content(rng, kind, n, w, h, dtype, maxv):
    """noise: one picture under fresh noise, frame i at exposure 0.7 + 0.15 i (the candidates differ in exposure: gains move); constant: frame
    i at level 60 + 30 i; black / clipped: all 0 / all the format's maximum -- nothing counts"""
    scale = (maxv + 1) // 256
    if kind == "noise":
        yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
        base = (70 + (xx * 3 + yy * 2) % 90 + 10 * cc) * scale
        f = base[None] + rng.integers(-8 * scale, 8 * scale + 1, (n, h, w, 3))
        f = f * (0.7 + 0.15 * np.arange(n))[:, None, None, None]
        return np.clip(np.floor(f), 0, maxv).astype(dtype)
    if kind == "constant":
        return (np.ones((n, h, w, 3), np.int64) * ((60 + 30 * np.arange(n)) * scale)[:, None, None, None]).astype(dtype)
    return np.full((n, h, w, 3), 0 if kind == "black" else maxv, dtype)


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
            row[3] = vs.Transform.of(0.0, 0.0, 1.0, -1.0)             # an integer shift
        if n_cand >= 5 and o % 2 == 1:
            cf[o, 4] = -1                                            # the list ends early
        ct.append(row)
    return cf, ct


@pytest.mark.parametrize("n_cand", [2, 16])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_stats_gains_and_gain_pass_equal_the_rule(gpu_vs, oracle, fmt, n_cand):
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(1000 * bits + n_cand)
    guard = 0x5A if bits == 8 else 0x5A5A
    n_src, n_out = 4, 3
    counted = moved = 0
    for si, (w, h) in enumerate(SHAPES):
        cf, ct = _cand_lists(vs, rng, n_out, n_cand, n_src, w, h)
        oct_ = [[_o(O, t) for t in row] for row in ct]
        for ki, kind in enumerate(KINDS):
            for step in (STEPS if kind == "noise" else (STEPS[(si + ki) % 3],)):
                p = vs.deflicker_params(step=step)
                src = _content(rng, kind, n_src, w, h, dtype, maxv)
                want_s = R.stats_batch(O, src, cf, oct_, bits, step)
                want_g = R.gains_batch(want_s, w, h, step)
                tgt = src[cf[:, 0]]
                want = R.gain_batch(tgt, want_g, maxv)
                if kind in ("black", "clipped"):                       # premise: nothing counts, the frames come back
                    assert not want_s.any() and (want_g[:, :3] == UNIT).all() and np.array_equal(want, tgt)
                counted += int(want_s[:, :, 0].sum())
                moved += int((want != tgt).sum())
                got_s = vs.exposure_stats_batch(src, cf, ct, params=p, fmt=code)
                assert np.array_equal(got_s, want_s), (w, h, kind, step)
                got_g = vs.exposure_gains_batch(got_s, w, h, params=p)
                assert np.array_equal(got_g, want_g), (w, h, kind, step, got_g.tolist(), want_g.tolist())
                got = vs.bgr_gain_batch(tgt, got_g, fmt=code)
                assert np.array_equal(got, want), (w, h, kind, step, int((got != want).sum()))
                if kind != "noise" or step != 1:
                    continue
                # pitched rows (odd: the dword variant falls back to the per-sample one), the destination inside a guard band that must stay
                # untouched; then rows that start on dwords
                for ss, ds in ((3 * w + 7, 3 * w + 5), (3 * w + 8, 3 * w + 4)):
                    assert np.array_equal(vs.exposure_stats_batch(src, cf, ct, params=p, fmt=code, src_stride=ss), want_s), (w, h, ss)
                    res, padded = vs.bgr_gain_batch(tgt, want_g, fmt=code, src_stride=ss, dst_stride=ds, guard=guard)
                    assert np.array_equal(res, want), (w, h, ss, ds)
                    assert (padded[:, :, 3 * w:] == guard).all()
    assert counted > 10000 and moved > 10000                           # the comparison was about counted pairs and changed samples


def test_default_parameters_and_the_frames_that_come_back(gpu_vs, oracle):
    vs, O = gpu_vs, oracle
    rng = np.random.default_rng(3)
    w, h = 260, 75
    src = _content(rng, "noise", 3, w, h, np.uint8, 255)
    ident, oid = vs.Transform.of(), O.Transform.of()
    # NULL parameters are step 4
    want, G = R.deflicker_frame(O, src, [0, 1, 2], [oid] * 3, 8, 255, 4)
    assert G[3] == 2 and not np.array_equal(want, src[0])
    st = vs.exposure_stats_batch(src, [[0, 1, 2]], [[ident] * 3])
    assert np.array_equal(st[0], np.array(R.stats_frame(O, src, [0, 1, 2], [oid] * 3, 8, 4), np.uint64))
    g = vs.exposure_gains_batch(st, w, h)
    assert g[0].tolist() == G
    assert np.array_equal(vs.bgr_gain_batch(src[:1], g)[0], want)
    # (a) one candidate, a list that ends at once, candidates outside the frame, too few pairs; (b) identical frames under identity maps
    far = vs.Transform.of(0, 0, 1000, 0)
    few = vs.Transform.of(0, 0, w - 4, 0)
    for cf, ct, m in (([1], [ident], 0), ([1, -1, 2], [ident] * 3, 0), ([1, 0, 2], [ident, far, far], 0), ([1, 0], [ident, few], 0), ([2, 2, 2, 2], [ident] * 4, 3)):
        st = vs.exposure_stats_batch(src, [cf], [ct])
        g = vs.exposure_gains_batch(st, w, h)
        assert g[0].tolist() == [UNIT, UNIT, UNIT, m], (cf, g)
        for kw in (dict(), dict(src_stride=3 * w + 1, dst_stride=3 * w + 3)):
            assert np.array_equal(vs.bgr_gain_batch(src[cf[0]][None], g, **kw)[0], src[cf[0]])
    # (c) constant frames of 100 and 200
    c = np.stack([np.full((9, 12, 3), 100, np.uint8), np.full((9, 12, 3), 200, np.uint8)])
    g = vs.exposure_gains_batch(vs.exposure_stats_batch(c, [[0, 1]], [[ident, ident]]), 12, 9)
    assert g[0].tolist() == [49152, 49152, 49152, 1]
    assert (vs.bgr_gain_batch(c[:1], g) == 150).all()
    # the ties of the two rounded divisions, through the device's 64-bit divisions
    row = [12 * 9, 65536, 65536, 65536, 65537, 65537, 65537, 0]
    assert vs.exposure_gains_batch(np.array([[[0] * 8, row]], np.uint64), 12, 9)[0].tolist() == [32769, 32769, 32769, 1]
    assert vs.exposure_gains_batch(np.array([[[0] * 8, row, row]], np.uint64), 12, 9)[0].tolist() == [32769, 32769, 32769, 2]


@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_device_memory_in_place_and_unaligned(gpu_vs, oracle, fmt):
    """device memory: more output frames than a kernel-argument block carries; the gain pass out of place and in place, on dword-aligned frames
    and on frames that start one element into their buffer with odd pitches (the per-sample variant); unit-gain frames among them"""
    import torch
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(5 + bits)
    w, h, n_src, n_out, n_cand = 132, 50, 6, 40, 5
    src = _content(rng, "noise", n_src, w, h, dtype, maxv)
    cf, ct = _cand_lists(vs, rng, n_out, n_cand, n_src, w, h)
    cf[7, 1:] = -1                                                   # a frame with unit gains
    want_s = R.stats_batch(O, src, cf, [[_o(O, t) for t in row] for row in ct], bits, 4)
    want_g = R.gains_batch(want_s, w, h, 4)
    assert (want_g[7, :3] == UNIT).all() and (want_g[:, :3] != UNIT).any(axis=1).sum() > 30
    want = R.gain_batch(src[cf[:, 0]], want_g, maxv)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda())
    for off, ss in ((0, 3 * w), (1, 3 * w + 7)):
        host = np.zeros(n_src * h * ss + 8, dtype)
        host[off:off + n_src * h * ss].reshape(n_src, h, ss)[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
        dsrc = as_t(host)
        dstats = torch.full((n_out * n_cand * 8 + 2,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
        dgains = torch.full((n_out * 4 + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        vs.exposure_stats_batch_device(dsrc.data_ptr() + off * esz, h * ss, n_src, w, h, ss, code, cf, ct, dstats.data_ptr() + 8)
        vs.exposure_gains_batch_device(dstats.data_ptr() + 8, n_out, n_cand, w, h, dgains.data_ptr() + 4)
        torch.cuda.synchronize()
        st = dstats.cpu().numpy().view(np.uint64)
        assert st[0] == 0x5A5A5A5A and st[-1] == 0x5A5A5A5A and np.array_equal(st[1:-1].reshape(n_out, n_cand, 8), want_s)
        gg = dgains.cpu().numpy().view(np.uint32)
        assert gg[0] == 0x5A5A5A5A and gg[-1] == 0x5A5A5A5A and np.array_equal(gg[1:-1].reshape(n_out, 4), want_g)
        # the targets laid out with the same offset and pitch; out of place into a guard-filled buffer, then in place
        guard = 0x5A if esz == 1 else 0x5A5A
        tbuf = np.zeros(n_out * h * ss + 8, dtype)
        tbuf[off:off + n_out * h * ss].reshape(n_out, h, ss)[:, :, :3 * w] = src[cf[:, 0]].reshape(n_out, h, 3 * w)
        dtgt, ddst = as_t(tbuf), as_t(np.full(n_out * h * ss + 8, guard, dtype))
        torch.cuda.synchronize()
        vs.bgr_gain_batch_device(dtgt.data_ptr() + off * esz, h * ss, n_out, w, h, ss, code, dgains.data_ptr() + 4, ddst.data_ptr() + off * esz, h * ss, ss)
        torch.cuda.synchronize()
        back = ddst.cpu().numpy().view(dtype)
        rows = back[off:off + n_out * h * ss].reshape(n_out, h, ss)
        assert np.array_equal(rows[:, :, :3 * w].reshape(n_out, h, w, 3), want), (off, ss)
        assert (rows[:, :, 3 * w:] == guard).all() and (back[:off] == guard).all() and (back[off + n_out * h * ss:] == guard).all()
        vs.bgr_gain_batch_device(dtgt.data_ptr() + off * esz, h * ss, n_out, w, h, ss, code, dgains.data_ptr() + 4, dtgt.data_ptr() + off * esz, h * ss, ss)
        torch.cuda.synchronize()
        back = dtgt.cpu().numpy().view(dtype)
        rows = back[off:off + n_out * h * ss].reshape(n_out, h, ss)
        assert np.array_equal(rows[:, :, :3 * w].reshape(n_out, h, w, 3), want), ("in place", off, ss)
        assert (rows[:, :, 3 * w:] == 0).all() and (back[:off] == 0).all() and (back[off + n_out * h * ss:] == 0).all()


K_SLOTS = 1 << 15                                                    # the parameter ring's slots


@pytest.mark.parametrize("n_cand,extra", [(16, 1), (2, 1)])
def test_one_output_frame_above_a_parameter_group(gpu_vs, oracle, n_cand, extra):
    """the candidate entries travel in groups of (kSlots / 2 / 4) / n_cand output frames: 256 at 16 candidates, 2048 at 2.  n_out = group + 1
    crosses the seam: the second group's statistics offset and ring span"""
    vs, O = gpu_vs, oracle
    group = (K_SLOTS // 2 // 4) // n_cand
    assert group == {16: 256, 2: 2048}[n_cand]
    n_out = group + extra
    w, h, n_src = 12, 9, 6
    rng = np.random.default_rng(n_cand)
    src = _content(rng, "noise", n_src, w, h, np.uint8, 255)
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    ct = [[vs.Transform.of(rng.uniform(-0.005, 0.005), rng.uniform(-0.01, 0.01), rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7)) for _ in range(n_cand)]
          for _ in range(n_out)]
    cf[group - 2:, 1] = (cf[group - 2:, 0] + 1) % n_src              # another frame on both sides of the seam
    p = vs.deflicker_params(step=1)
    want_s = R.stats_batch(O, src, cf, [[_o(O, t) for t in row] for row in ct], 8, 1)
    want_g = R.gains_batch(want_s, w, h, 1)
    assert (want_s[group - 2:, 1, 0] > 0).all() and (want_g[group - 2:, :3] != UNIT).any(axis=1).all()
    got_s = vs.exposure_stats_batch(src, cf, ct, params=p)
    bad = [o for o in range(n_out) if not np.array_equal(got_s[o], want_s[o])]
    assert not bad, (bad[:8], len(bad))
    got_g = vs.exposure_gains_batch(got_s, w, h, params=p)
    assert np.array_equal(got_g, want_g)
    assert np.array_equal(vs.bgr_gain_batch(src[cf[:, 0]], got_g), R.gain_batch(src[cf[:, 0]], want_g, 255))


def test_argument_errors_and_the_handle_s_boundary(gpu_vs):
    vs = gpu_vs
    src = np.full((3, 32, 48, 3), 90, np.uint8)
    t = vs.Transform.of(0, 0, 3, 2)
    assert vs.exposure_stats_batch(src, [[0, 1]], [[t, t]]).shape == (1, 2, 8)
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 0
        vs.exposure_stats_batch(src, np.zeros((1, 0), np.int32), [[]])
    with pytest.raises(vs.VsError, match="error -1"):               # n_cand 17
        vs.exposure_stats_batch(src, [[0] * 17], [[t] * 17])
    with pytest.raises(vs.VsError, match="error -1"):               # a source index >= n_src
        vs.exposure_stats_batch(src, [[0, 3]], [[t, t]])
    with pytest.raises(vs.VsError, match="error -1"):               # candidate 0 is the frame itself: it cannot be missing
        vs.exposure_stats_batch(src, [[-1, 1]], [[t, t]])
    # a negative index ends the list: what lies behind it is not read, not even to be checked
    assert not vs.exposure_stats_batch(src, [[0, -1, 99]], [[t, t, t]]).any()
    with pytest.raises(vs.VsError, match="error -1"):               # a gain outside 16384 .. 65536 in host memory
        vs.bgr_gain_batch(src[:1], [[UNIT, 65537, UNIT, 0]])
    with pytest.raises(vs.VsError, match="error -1"):
        vs.bgr_gain_batch(src[:1], [[16383, UNIT, UNIT, 0]])
    assert np.array_equal(vs.bgr_gain_batch(src[:1], [[16384, 65536, UNIT, 99]])[0, 0, 0], [45, 180, 90])
    s = vs.Stabilizer(device=0, lag=6)
    assert s.get_deflicker() == 0
    for step, ok in ((0, False), (1, True), (64, True), (65, False)):
        p = vs.deflicker_params(step=step)
        if ok:
            s.set_deflicker(2, p)
            assert vs.exposure_stats_batch(src, [[0, 1]], [[t, t]], params=p).shape == (1, 2, 8)
        else:
            with pytest.raises(vs.VsError, match="error -1"):
                s.set_deflicker(3, p)
            with pytest.raises(vs.VsError, match="error -1"):
                vs.exposure_stats_batch(src, [[0, 1]], [[t, t]], params=p)
            with pytest.raises(vs.VsError, match="error -1"):
                vs.exposure_gains_batch(np.zeros((1, 2, 8), np.uint64), 48, 32, params=p)
        assert s.get_deflicker() == 2 or step == 0
    with pytest.raises(vs.VsError, match="error -1"):               # ahead > lag
        s.set_deflicker(7)
    with pytest.raises(vs.VsError, match="error -1"):
        s.set_deflicker(-1)
    s.set_deflicker(6)
    assert s.get_deflicker() == 6
    s.set_deflicker(0)
    assert s.get_deflicker() == 0
    assert vs.Stabilizer(device=0, warp_mode=vs.WARP_LANCZOS2, deflicker=3).get_deflicker() == 3        # every warp mode


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------
_clips = {}


def _flicker_clip(n, seed, bits=8, w=W, h=H):
    """a synth clip under an exposure drift: 1.2 % up per frame with 0.4 % of seeded jitter, falling back every 24 frames.  (The aligner is not
    robust to exposure changes -- per-frame jumps of 5 % make most alignments of such small frames fail -- so the drift is what keeps most lists
    whole; the fall makes an alignment fail, which ends the lists in front of it early.)"""
    key = (n, seed, bits, w, h)
    if key not in _clips:
        from video_stabilizer_amd import synth
        maxv = (1 << bits) - 1
        a = synth.make_clip(w, h, n, seed=seed, channels=3, bits=bits, jitter_b=0.01)[0]
        g = 0.88 * 1.012 ** (np.arange(n) % 24) * (1 + 0.004 * np.random.default_rng(seed + 500).uniform(-1, 1, n))
        _clips[key] = np.clip(np.floor(a.astype(np.float64) * g[:, None, None, None] + 0.5), 0, maxv).astype(a.dtype)
    return _clips[key]


def _kernel_level(vs, O, frames, fmt, ahead, step, off, lag):
    """the engine's outputs rebuilt: the deflicker-off outputs `off` put through the kernel-level calls, with candidates composed here from a
    capi.Aligner's measurements.  The statistics are checked against the restatement on the way"""
    n, h, w, _ = frames.shape
    bits = 8 if frames.dtype == np.uint8 else 10
    status, meas = vs.Aligner(device=0, select_mode=vs.SELECT_DEVICE).align_batch(frames, fmt=fmt)
    p = vs.deflicker_params(step=step)
    ks = sorted(off)
    lists = [EM.lookahead_candidates(vs, k, ahead, meas, status) for k in ks]
    ended_early = sum(l[0][-1] < 0 for l in lists)
    st = vs.exposure_stats_batch(frames, [l[0] for l in lists], [l[1] for l in lists], params=p, fmt=fmt)
    want_s = R.stats_batch(O, frames, [l[0] for l in lists], [[_o(O, t) for t in l[1]] for l in lists], bits, step)
    assert np.array_equal(st, want_s)
    g = vs.exposure_gains_batch(st, w, h, params=p)
    assert np.array_equal(g, R.gains_batch(want_s, w, h, step))
    outs = vs.bgr_gain_batch(np.stack([off[k] for k in ks]), g, fmt=fmt)
    return {k: outs[i] for i, k in enumerate(ks)}, g, ended_early


CASES = {"cv": dict(), "cv_fill_blend": dict(border_fill=3, fill_blend=(3, 1)), "cv_deblur_denoise": dict(deblur=3, denoise=2),
         "cv_all": dict(border_fill=3, fill_blend=(2, 1), deblur=3, denoise=3), "lanczos2": dict(warp_mode=0), "cv_10bit": dict(border_fill=2)}
LAG = 5


def _case_kw(vs, case):
    kw = dict(device=0, select_mode=vs.SELECT_DEVICE, lag=LAG, crop_pixels=0 if "border_fill" in CASES[case] else 8)
    kw.update(CASES[case])
    return kw


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_route_equals_the_kernel_level_calls(gpu_vs, oracle, case):
    """process frame by frame == process_batch (one call; split calls) == device memory == the deflicker-off output through the kernel-level calls;
    with fill + blend, deblur and denoise on and off, once with a Lanczos2 warp, once in 10 bits; failed alignments in the middle"""
    import torch
    vs, O = gpu_vs, oracle
    bits = 10 if case == "cv_10bit" else 8
    frames = _flicker_clip(27, 11, bits)
    n = len(frames)
    fmt = vs.FMT_BGR8 if bits == 8 else vs.FMT_BGR10
    kw = _case_kw(vs, case)
    crop = kw["crop_pixels"]
    s_on, s_off = [], []
    off = frame_by_frame(vs.Stabilizer(**kw), frames, s_off)
    want, gains, ended_early = _kernel_level(vs, O, frames, fmt, 4, 4, off, LAG)
    assert ended_early > 0, "the fall no longer makes an alignment fail: the test input has to change"
    assert (gains[:, 3] == 4).sum() > 5 and (np.abs(gains[:, :3].astype(np.int64) - UNIT) > 300).any()
    kw = dict(kw, deflicker=4)
    ref = frame_by_frame(vs.Stabilizer(**kw), frames, s_on)
    assert s_on == s_off                                             # transforms, state and has_output do not depend on the setting
    assert sorted(ref) == sorted(want)
    for k in want:
        assert np.array_equal(ref[k], want[k]), (k, int((ref[k] != want[k]).sum()))
    assert sum(int((ref[k] != off[k]).sum()) for k in ref) > 0.2 * sum(ref[k].size for k in ref)      # the pass did something
    out, has = vs.Stabilizer(**kw).process_batch(frames)
    assert [i - LAG for i, hh in enumerate(has) if hh] == sorted(ref)
    for i, hh in enumerate(has):
        if hh:
            assert np.array_equal(out[i], ref[i - LAG]), i
    # split calls: queued frames become buffers of the handle between the calls and are candidates of the next call's jobs
    st = vs.Stabilizer(**kw)
    pos = 0
    for m in (3, 1, 9, 2, n - 15):
        o, hs = st.process_batch(frames[pos:pos + m])
        for i, hh in enumerate(hs):
            if hh:
                assert np.array_equal(o[i], ref[pos + i - LAG]), (pos, i)
        pos += m
    assert pos == n
    # device-resident frames
    dev = torch.from_numpy(frames.view(np.int16) if bits != 8 else frames).cuda()
    dout = torch.zeros((n, H - 2 * crop, W - 2 * crop, 3), dtype=dev.dtype, device="cuda")
    st = vs.Stabilizer(**kw)
    r, hs = st.process_batch_device(dev.data_ptr(), n, W, H, fmt, dout.data_ptr())
    torch.cuda.synchronize()
    res = dout.cpu().numpy().view(frames.dtype)
    assert r == len(ref)
    for i, hh in enumerate(hs):
        if hh:
            assert np.array_equal(res[i], ref[i - LAG]), i


def test_switching_in_mid_clip_and_a_reset(gpu_vs):
    """off by default; off after on is a handle that never had it; on in mid-sequence takes effect with the next output frame and equals a handle
    that had it from the start.  After a reset nothing that came before is a candidate"""
    vs = gpu_vs
    frames = _flicker_clip(27, 11)
    kw = dict(device=0, lag=LAG, crop_pixels=8)
    a, b, c = vs.Stabilizer(**kw), vs.Stabilizer(**kw), vs.Stabilizer(deflicker=3, **kw)
    changed = False
    for i, f in enumerate(frames):
        if i == 7:
            a.set_deflicker(3)
        if i == 18:
            a.set_deflicker(0)
        oa, ob, oc = a.process(f), b.process(f), c.process(f)
        assert (oa is None) == (ob is None) == (oc is None)
        if oa is None:
            continue
        if 7 <= i < 18:
            assert np.array_equal(oa, oc), i
            changed |= not np.array_equal(oa, ob)
        else:
            assert np.array_equal(oa, ob), i
    assert changed
    st = vs.Stabilizer(deflicker=4, **kw)
    for f in frames[:9]:
        st.process(f)
    st.reset()
    got = frame_by_frame(st, frames[14:])
    want = frame_by_frame(vs.Stabilizer(deflicker=4, **kw), frames[14:])
    assert sorted(got) == sorted(want) and len(want) > 3 and all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("extra", [dict(), dict(deblur=3, denoise=2, border_fill=2, fill_blend=(2, 1))], ids=["deflicker", "all_passes"])
def test_chunked_and_pipelined_batches(gpu_vs, monkeypatch, extra):
    """a device-resident clip long enough for the time chunks (statistics, warps and gain pass on their own stream, the next chunk's alignment
    prefetched) and a host batch long enough for the upload / compute / download pipeline (the downloader's event covers the gain pass), against
    process_batch calls that stay below both thresholds"""
    import torch
    vs = gpu_vs
    n = 100
    frames = _flicker_clip(n, 9)
    monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(37 * W * H * 3))  # host batches: upload chunks of 37 frames (read at every call)
    kw = dict(device=0, lag=6, crop_pixels=0, deflicker=4, **extra)
    st = vs.Stabilizer(**kw)
    ref = np.zeros_like(frames)
    ref_has = []
    for p in range(0, n, 20):                                        # short calls: one chunk each, no overlap
        o, hs = st.process_batch(frames[p:p + 20])
        ref[p:p + 20] = o
        ref_has += hs
    plain, _ = vs.Stabilizer(**dict(kw, deflicker=0)).process_batch(frames[:20])
    assert not np.array_equal(plain, ref[:20])
    out, has = vs.Stabilizer(**kw).process_batch(frames)            # host memory, one call
    assert has == ref_has and np.array_equal(out, ref)
    dev = torch.from_numpy(frames).cuda()
    dout = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    st = vs.Stabilizer(**kw)
    for _ in range(2):                                               # (the second call reuses the block)
        st.reset()
        dout.zero_()
        r, hs = st.process_batch_device(dev.data_ptr(), n, W, H, vs.FMT_BGR8, dout.data_ptr())
        torch.cuda.synchronize()
        assert hs == ref_has and np.array_equal(dout.cpu().numpy(), ref)


@pytest.mark.parametrize("case", ["plain", "all_passes"])
def test_process_clips_and_size_change(gpu_vs, case):
    """process_clips on host and device memory against one frame-by-frame handle per clip; no frame of the next clip is ever a candidate; a size
    change starts a new clip"""
    import torch
    vs = gpu_vs
    n_clips, fpc = 4, 24
    clips = [_flicker_clip(fpc, 20 + c) for c in range(n_clips)]
    kw = dict(device=0, lag=LAG, crop_pixels=8, deflicker=4)
    if case == "all_passes":
        kw.update(border_fill=3, fill_blend=(2, 1), crop_pixels=0, deblur=3, denoise=2)
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
    off = frame_by_frame(vs.Stabilizer(**dict(kw, deflicker=0)), clips[0])
    assert any(not np.array_equal(off[k], ref[0][k]) for k in off)   # the pass does something on these clips
    for c in range(n_clips):
        for i in range(fpc):
            assert bool(has[c * fpc + i]) == (i - LAG in ref[c])
            if has[c * fpc + i]:
                assert np.array_equal(out[c * fpc + i], ref[c][i - LAG]), (c, i)
                assert np.array_equal(dres[c * fpc + i], ref[c][i - LAG]), (c, i)
    small = _flicker_clip(14, 31, w=128, h=96)
    st = vs.Stabilizer(**kw)
    for f in clips[0][:9]:
        st.process(f)
    got = frame_by_frame(st, small)
    want = frame_by_frame(vs.Stabilizer(**kw), small)
    assert sorted(got) == sorted(want) and len(want) > 3 and all(np.array_equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("throwing", [False, True])
def test_deflickered_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    """every allocation of a deflickered process_batch failed once, both signs; the handle recovers.  A handle whose deflicker was switched on and
    off again makes the allocations of one that never had it (counted on calls that succeed), and deflicker on makes exactly one more: the
    statistics + gains block"""
    vs = gpu_vs
    frames = _flicker_clip(16, 7)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    kw = dict(device=0, lag=4, smoother_memory=2, crop_pixels=8)

    def off_again():
        s = vs.Stabilizer(deflicker=3, **kw)
        s.set_deflicker(0)
        return s
    def allocations(make):
        """how many allocations one call on a fresh handle makes (none of them failed)"""
        h = make()
        vs.test_fail_alloc(1 << 30)
        call(h)
        return vs.test_fail_alloc(0)
    n_never, n_off, n_on = allocations(lambda: vs.Stabilizer(**kw)), allocations(off_again), allocations(lambda: vs.Stabilizer(deflicker=3, **kw))
    assert n_off == n_never and n_on == n_off + 1
    on = walk(vs, lambda: vs.Stabilizer(deflicker=3, **kw), call, n_on, throwing)
    print("deflickered process_batch: %d allocations failed one by one (%s); %d with deflicker off" % (on, "throwing" if throwing else "error code", n_off))
    assert on == n_on


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
    src = np.clip((base[None] + rng.integers(-6, 7, (n_src, h, w, 3)) * ((maxv + 1) // 256)) * (0.8 + 0.1 * np.arange(n_src))[:, None, None, None], 0, maxv).astype(dtype)
    cf = np.array([[4, 0, -1, -1], [1, -1, -1, -1], [2, 3, 4, 0], [3, 4, -1, 2], [0, 1, 2, 3]], np.int32)
    ct = [[G.Transform.of(rng.uniform(-0.002, 0.002), rng.uniform(-0.003, 0.003), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)) for _ in range(4)] for _ in range(5)]
    ct[0] = [G.Transform.of(0.0, 0.0, 5000.0 + 100 * c, -3000.0) for c in range(4)]          # output 0: every map leaves the frame
    st = G.exposure_stats_batch(src, cf, ct, fmt=fmt)
    g = G.exposure_gains_batch(st, w, h)
    put(st, g, G.bgr_gain_batch(src, g, fmt=fmt), G.bgr_gain_batch(src, g, fmt=fmt, src_stride=3 * w + 7, dst_stride=3 * w + 5))
clip = synth.make_clip(160, 128, 20, seed=5, channels=3)[0]
clip = (clip * (0.85 * 1.012 ** np.arange(20))[:, None, None, None]).astype(np.uint8)
clip = np.concatenate([clip[:9], synth.make_clip(160, 128, 3, seed=77, channels=3)[0], clip[9:]])
for kw in (dict(deflicker=4), dict(deflicker=4, denoise=2, deblur=3, border_fill=3, crop_pixels=0), dict(deflicker=2, warp_mode=G.WARP_LANCZOS2)):
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
def test_deflicker_does_not_depend_on_what_fresh_allocations_contain(gpu_vs, byte):
    # one child process per fill byte; every case compares with the zero-filled run (the first case pays for both)
    assert _digest(byte) == _digest(0)


def test_video_test_deflicker_writes_what_the_library_returns(gpu_vs, tmp_path):
    frames = _flicker_clip(27, 11)
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("flicker_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    exe = os.path.join(ROOT, "apps", "bin", "vs_video_test")
    r = subprocess.run([exe, str(d), str(tmp_path / "out"), "--crop", "0", "--deflicker", "4", "--deflicker-step", "2", "--chunk", "13"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    st = gpu_vs.Stabilizer(device=0, crop_pixels=0, deflicker=4, deflicker_params=gpu_vs.deflicker_params(step=2))
    want = np.stack([o for o in (st.process(f) for f in frames) if o is not None])
    got = np.fromfile(tmp_path / "out" / ("processed_" + raw.name), np.uint8).reshape(-1, H, W, 3)
    assert np.array_equal(got, want)
    st0 = gpu_vs.Stabilizer(device=0, crop_pixels=0)
    assert not np.array_equal(want, np.stack([o for o in (st0.process(f) for f in frames) if o is not None]))
    r = subprocess.run([exe, str(d), str(tmp_path / "out2"), "--deflicker", "4", "--deflicker-step", "65"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "vs_stabilizer_set_deflicker" in r.stderr
