"""The rolling-shutter kernel (vs_rolling.hip) on hostile input: NaN, infinite, singular, near-singular, saturating and quarter-turn motions,
rint ties on the row terms, samples above the format's maximum, the C ABI's group seam, an allocation failure at the pass's scratch -- bit for
bit against the rule's restatement (tests/_rolling_ref.py).  Inputs: tests/_hostile_maps.py; every case asserts its premise on the CPU
restatement before it looks at the GPU.

All kernel-level calls work on DEVICE memory with the destination inside a guard band on all four sides (the host-memory form copies only
the rows' own bytes back)."""
import ctypes as C

import numpy as np
import pytest

import _fill_ref as RF
import _hostile_maps as HM
import _rolling_ref as R
from _stab_routes import walk

pytestmark = pytest.mark.gpu

G = 3
IDENT = (0.0, 0.0, 0.0, 0.0)
FORMATS = HM.FORMATS


def _dev_rolling(vs, src, cf, maps, fmt, rho, ss=None, ds=None, odd=False):
    """vs_bgr_rolling_batch on device memory, the destination frames G rows apart inside a guard-filled buffer -> (n_out, h, w, 3).
    odd: source and destination start one element into their buffers (8-bit: not on a dword -- the one-pixel form)"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    ss = 3 * w if ss is None else ss
    ds = 3 * w if ds is None else ds
    off = 1 if odd else 0
    host = np.zeros(n_src * h * ss + 8, dtype)
    host[off:off + n_src * h * ss].reshape(n_src, h, ss)[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out, n_cand = idx.shape
    assert n_cand == 2
    flat = [vs.Transform.of(*t) for row in maps for t in row]
    assert len(flat) == n_out * 2
    arr = (vs.Transform * len(flat))(*flat)
    dfs = (h + 2 * G) * ds
    guard = 0x5A if esz == 1 else 0x5A5A
    dhost = np.full(n_out * dfs + 8, guard, dtype)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda())
    dsrc, ddst = as_t(host), as_t(dhost)
    torch.cuda.synchronize()
    p = vs.rolling_params(readout=rho)
    vs._check(vs.lib().vs_bgr_rolling_batch(C.c_void_p(dsrc.data_ptr() + off * esz), h * ss, n_src, w, h, ss, fmt, n_out,
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), arr, C.byref(p),
                                            C.c_void_p(ddst.data_ptr() + (G * ds + off) * esz), dfs, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    assert (back[:off] == guard).all() and (back[off + n_out * dfs:] == guard).all()
    frames = back[off:off + n_out * dfs].reshape(n_out, h + 2 * G, ds)
    res = frames[:, G:G + h, :3 * w].reshape(n_out, h, w, 3).copy()
    frames[:, G:G + h, :3 * w] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination frame were written"
    assert (frames[:, G + h:] == guard).all(), "rows below a destination frame were written"
    assert (frames[:, G:G + h, 3 * w:] == guard).all(), "the tail of a destination row was written"
    return res


def _ref(vs, src, cf, maps, rho, maxv):
    with np.errstate(all="ignore"):
        return R.rolling_batch(HM.cvinv(vs), src, cf, [[vs.Transform.of(*t) for t in row] for row in maps], rho, maxv)


def _outside_share(vs, tup, w, h, rho):
    """share of the pixels with a tap that the border clamp moves"""
    with np.errstate(all="ignore"):
        X, Y = R.positions(HM.cvinv(vs)(vs.Transform.of(*tup), w, h), w, h, rho)
    sx, sy = X >> 5, Y >> 5
    return float(((sx < 0) | (sx + 1 > w - 1) | (sy < 0) | (sy + 1 > h - 1)).mean())


@pytest.mark.parametrize("shape", [(64, 48), (67, 21)], ids=["64x48", "67x21"])          # (four pixels per lane; the one-pixel form)
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_hostile_motions(gpu_vs, fmt, shape):
    """(f): each hostile map as the motion.  Premises: the huge shifts put every tap outside the frame, the quarter turns and the singular map
    some of them (the clamp is live on whole frames and across frames); a NaN row matrix is position (0, 0) -- every row but none of a finite motion's; the restatement keeps (e) on all of them"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = shape
    rng = np.random.default_rng(3 * bits + w)
    src = rng.integers(maxv // 8, maxv - maxv // 8, (3, h, w, 3)).astype(dtype)
    hostile = dict(HM.HOSTILE)
    hostile.update(HM.FILL_EXTREME)
    hostile["row0_trap"] = HM.row0_trap(vs, w, h)
    names = sorted(hostile)
    maps = [[IDENT, hostile[n]] for n in names]
    cf = np.array([[i % 3, 0] for i in range(len(maps))], np.int32)
    for n in ("p1e300", "t_1e300", "tx_6e5", "tx_m3e6", "ty_3e6", "inf_TX"):
        assert _outside_share(vs, hostile[n], w, h, 1.0) > 0.9, n    # every pixel has a clamped tap (but on an odd frame's middle row, tau == 0)
    for n in ("near_1e-6", "rot180_zoom2", "rot90_zoom05", "singular"):
        assert 0.05 < _outside_share(vs, hostile[n], w, h, 1.0) < 0.9, n
    for rho in (1.0, -0.7):
        want = _ref(vs, src, cf, maps, rho, maxv)
        i = names.index("nan_A")
        assert (want[i] == src[cf[i, 0]][0, 0]).all()                # cvRound(NaN) = 0 in all four terms: pixel (0, 0) everywhere
        for i in range(len(maps)):
            f = src[cf[i, 0]]
            assert (want[i].reshape(-1, 3).min(0) >= f.reshape(-1, 3).min(0)).all() and (want[i].reshape(-1, 3).max(0) <= f.reshape(-1, 3).max(0)).all()
        got = _dev_rolling(vs, src, cf, maps, code, rho)
        bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (rho, bad)
        got = _dev_rolling(vs, src, cf, maps, code, rho, ss=3 * w + 7, ds=3 * w + 5, odd=True)
        bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, ("unaligned", rho, bad)


@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_rint_ties_on_the_row_terms(gpu_vs, fmt):
    """h = 16 and rho = 1: tau(y) = (2 y - 15) / 32 exactly.  A shift of (-k / 64, -m / 64) with odd k, m gives M2 = k / 64, M5 = m / 64, and
    tau M2 * 1024 = k (2 y - 15) / 2: every row origin's argument is a half-integer.  Premise asserted: ties-to-even and round-half-up
    differ on half the rows or so, in both terms"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = 68, 16
    rng = np.random.default_rng(bits)
    src = rng.integers(0, maxv + 1, (2, h, w, 3)).astype(dtype)
    maps = [[IDENT, (0.0, 0.0, -1.0 / 64, -3.0 / 64)], [IDENT, (0.0, 0.0, 5.0 / 64, -1.0 / 64)], [IDENT, (0.0, 0.0, -33.0 / 64, 7.0 / 64)]]
    cf = np.array([[0, 0], [1, 0], [0, 1]], np.int32)
    ys = np.arange(h, dtype=np.float64)
    for _, tup in maps:
        r = R.row_matrices(HM.cvinv(vs)(vs.Transform.of(*tup), w, h), h, 1.0)
        for v in ((r[:, 1] * ys + r[:, 2]) * 1024.0, (r[:, 4] * ys + r[:, 5]) * 1024.0):
            assert (v % 1 == 0.5).all()
            assert 0.25 < (np.rint(v) != np.floor(v + 0.5)).mean() < 0.75
    want = _ref(vs, src, cf, maps, 1.0, maxv)
    assert np.array_equal(_dev_rolling(vs, src, cf, maps, code, 1.0), want)
    assert np.array_equal(_dev_rolling(vs, src, cf, maps, code, 1.0, ss=3 * w + 1, ds=3 * w + 3, odd=True), want)


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples.  Premises: the blend's saturation is live (the result
    under max_value 65535 differs), a corrected sample never exceeds the maximum, and a frame without motion keeps its samples as they came"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((131, 37), (132, 20)):
        src = rng.integers(0, maxv + 1, (2, h, w, 3)).astype(dtype)
        for f in src:
            f[rng.random((h, w)) < 0.08] = 65535
            f[rng.random((h, w, 3)) < 0.05] = maxv + 1
        maps = [[IDENT, (0.0, 0.001, 0.3, 0.6)], [IDENT, (0.001, 0.0, -4.4, 2.2)], [IDENT, IDENT]]
        cf = np.array([[0, 1], [1, 0], [0, -1]], np.int32)
        want = _ref(vs, src, cf, maps, 0.9, maxv)
        loose = _ref(vs, src, cf, maps, 0.9, 65535)
        assert not np.array_equal(want[:2], loose[:2]) and want[:2].max() == maxv
        assert np.array_equal(want[2], src[0]) and want[2].max() == 65535
        got = _dev_rolling(vs, src, cf, maps, code, 0.9)
        assert np.array_equal(got, want), (w, h, int((got != want).sum()))


K_SLOTS = 1 << 15                                                    # the parameter ring's slots (frames per group)


def test_the_second_group_of_a_long_call(gpu_vs):
    """vs_bgr_rolling_batch uploads its two entries per frame in groups of (kSlots / 2 / 4) / 2 = 2048 output frames; n_out = 2051 crosses
    the seam: the second group's destination offset and ring span"""
    vs = gpu_vs
    group = (K_SLOTS // 2 // 4) // 2
    n_out = group + 3
    w, h, n_src = 12, 9, 4
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (n_src, h, w, 3)).astype(np.uint8)
    cf = np.stack([rng.integers(0, n_src, n_out), np.where(rng.random(n_out) < 0.1, -1, 0)], axis=1).astype(np.int32)
    cf[group - 2:, 1] = 0
    maps = [[IDENT, (rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(-3, 3), rng.uniform(-3, 3))] for _ in range(n_out)]
    want = _ref(vs, src, cf, maps, 1.0, 255)
    assert all((want[o] != src[cf[o, 0]]).any() for o in range(group - 2, n_out))
    got = _dev_rolling(vs, src, cf, maps, vs.FMT_BGR8, 1.0)
    bad = [o for o in range(n_out) if not np.array_equal(got[o], want[o])]
    assert not bad, (bad[:8], len(bad))


CHILD = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
import numpy as np
from video_stabilizer_amd import capi as G, synth
dig = hashlib.sha256()
rng = np.random.default_rng(5)
for dtype, maxv, fmt, (w, h) in ((np.uint8, 255, G.FMT_BGR8, (260, 33)), (np.uint16, 1023, G.FMT_BGR10, (129, 65)), (np.uint8, 255, G.FMT_BGR8, (9, 1))):
    img = rng.integers(0, maxv + 1, (3, h, w, 3)).astype(dtype)
    t = [[G.Transform.of(), G.Transform.of(0.01, -0.02, 7.5, -3.0)], [G.Transform.of(), G.Transform.of()]]
    for kw in (dict(), dict(src_stride=3 * w + 7, dst_stride=3 * w + 5)):
        dig.update(G.rolling_batch(img, [[0, 1], [2, -1]], t, params=G.rolling_params(readout=0.9), fmt=fmt, **kw).tobytes())
clip = np.maximum(synth.make_clip(160, 128, 14, seed=5, channels=3)[0], 1)
for kw in (dict(crop_pixels=8), dict(crop_pixels=0, border_fill=3, denoise=2, inpaint=1)):
    kw = dict(dict(device=0, lag=4, rolling_shutter=0.8), **kw)
    s = G.Stabilizer(**kw)
    for fr in clip:
        o = s.process(fr)
        dig.update(b"-" if o is None else o.tobytes())
    out, has = G.Stabilizer(**kw).process_batch(clip)
    dig.update(repr(has).encode() + out[np.array(has, bool)].tobytes())
print("DIGEST", dig.hexdigest())
"""


def test_rolling_does_not_depend_on_what_fresh_allocations_contain(gpu_vs):
    """one child process per fill byte of every fresh device allocation (VS_TEST_POISON_ALLOC): the kernel-level call and the engine with the
    pass on give the same bytes"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    for byte in (255, 0):
        env = dict(os.environ, VS_TEST_POISON_ALLOC=str(byte), VS_TEST_HOOKS="1")
        out = subprocess.run([sys.executable, "-c", CHILD % {"root": root}], cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        digests.append([line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1])
    assert digests[0] == digests[1]


@pytest.mark.parametrize("throwing", [False, True])
def test_corrected_process_batch_survives_every_allocation_failure(gpu_vs, throwing):
    """every allocation of a process_batch call with the pass on is failed once (vs_test_fail_alloc), the pass's scratch among them: the call
    reports it, the next call on the handle equals a fresh handle's"""
    vs = gpu_vs
    from video_stabilizer_amd import synth
    frames = np.maximum(synth.make_clip(160, 128, 12, seed=7, channels=3, bits=8)[0], 1)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    kw = dict(device=0, lag=4, smoother_memory=2, crop_pixels=8)

    def allocations(make):
        h = make()
        vs.test_fail_alloc(1 << 30)
        call(h)
        return vs.test_fail_alloc(0)
    allocations(lambda: vs.Stabilizer(**kw))                         # (the process-wide staging pool fills on the first call)
    n_off, n_on = allocations(lambda: vs.Stabilizer(**kw)), allocations(lambda: vs.Stabilizer(rolling_shutter=0.7, **kw))
    assert n_on == n_off + 1                                         # the scratch block joins the protocol
    fired = walk(vs, lambda: vs.Stabilizer(rolling_shutter=0.7, **kw), call, n_on, throwing)
    assert fired == n_on
