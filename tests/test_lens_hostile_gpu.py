"""The remap and the lens map (vs_remap.hip) on hostile input: maps that hold the extremes of int32 and every position around the frame's
edges, samples above the format's maximum, a lens whose denominator vanishes on a ring, poisoned allocations, every allocation of a call
failed once -- bit for bit against the rule's restatement (tests/_lens_ref.py).  Every case asserts its premise on the CPU restatement before
it looks at the GPU.

The kernel-level calls work on DEVICE memory with source, map and destination inside guard bands on all four sides (the host-memory form
copies only the rows' own bytes back).  The source's guard holds a value no frame sample has: a tap that strays into it shows in the result."""
import ctypes as C

import numpy as np
import pytest

import _lens_ref as L
from _stab_routes import walk
from test_lens_cpu import COEFFS

pytestmark = pytest.mark.gpu

G = 3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12)}


def _banded(a, row_elems, stride, guard, lead):
    """frames (n, rows, row_elems) -> a flat buffer: `lead` elements in front, every frame G guard rows above and below, rows of `stride`"""
    n, rows, _ = a.shape
    buf = np.full(lead + n * (rows + 2 * G) * stride + 8, guard, a.dtype)
    buf[lead:lead + n * (rows + 2 * G) * stride].reshape(n, rows + 2 * G, stride)[:, G:G + rows, :row_elems] = a
    return buf


def _dev_remap(vs, src, pos, fmt, border, src_guard, aligned=False):
    """vs_bgr_remap_batch on device memory, all three buffers banded -> (n, oh, ow, 3).  aligned: the buffers start four elements into their
    allocations and the destination's rows are dwords apart (the four-pixel form where ow is a multiple of 4); else one element in, odd
    pitches (8-bit: the one-pixel form)"""
    import torch
    src = np.ascontiguousarray(src)
    n, h, w, _ = src.shape
    oh, ow, _ = pos.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    lead, pad = (4, (8, 4, 4)) if aligned else (1, (7, 5, 3))
    ss, ds, ms = 3 * w + pad[0], 3 * ow + pad[1], 2 * ow + pad[2]
    guard = 0x5A if esz == 1 else 0x5A5A
    hsrc = _banded(src.reshape(n, h, 3 * w), 3 * w, ss, src_guard, lead)
    hmap = _banded(np.ascontiguousarray(pos, np.int32).reshape(1, oh, 2 * ow), 2 * ow, ms, 0x7FFFFFF1, lead)
    hdst = _banded(np.full((n, oh, 3 * ow), guard, dtype), 3 * ow, ds, guard, lead)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda())
    dsrc, dmap, ddst = as_t(hsrc), as_t(hmap), as_t(hdst)
    torch.cuda.synchronize()
    vs._check(vs.lib().vs_bgr_remap_batch(C.c_void_p(dsrc.data_ptr() + (lead + G * ss) * esz), (h + 2 * G) * ss, n, w, h, ss, fmt,
                                          C.c_void_p(dmap.data_ptr() + (lead + G * ms) * 4), ms, ow, oh, border,
                                          C.c_void_p(ddst.data_ptr() + (lead + G * ds) * esz), (oh + 2 * G) * ds, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    assert np.array_equal(dsrc.cpu().numpy().view(dtype), hsrc) and np.array_equal(dmap.cpu().numpy(), hmap)      # inputs are only read
    frames = back[lead:lead + n * (oh + 2 * G) * ds].reshape(n, oh + 2 * G, ds)
    res = frames[:, G:G + oh, :3 * ow].reshape(n, oh, ow, 3).copy()
    frames[:, G:G + oh, :3 * ow] = guard
    assert (back == guard).all(), "the destination was written outside its frames' rows"
    return res


def _edge_values(w):
    """INT_MIN, INT_MAX, -33, -32, -1, 0, 32 (w - 1), 32 (w - 1) + 1 and 32 w, each with fractions 0 and 31"""
    base = [INT_MIN, INT_MAX, -33, -32, -1, 0, 32 * (w - 1), 32 * (w - 1) + 1, 32 * w]
    return sorted(set(base + [v & ~31 for v in base] + [v | 31 for v in base]))


@pytest.mark.parametrize("shape", [(2, 2), (7, 5), (64, 8)], ids=["2x2", "7x5", "64x8"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_maps_that_hold_the_extremes(gpu_vs, fmt, shape):
    """every pair of the edge values, X by Y, as one map, in the one-pixel form and (the map repeated sideways to a multiple of 4 columns) in
    the four-pixel form.  Premises: both int extremes and both fractions occur in both coordinates, most positions have a tap outside, the
    restatement keeps (b) under the clamp border and gives 0 under the constant border wherever all four taps are outside"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = shape
    rng = np.random.default_rng(bits + w)
    src = rng.integers(maxv // 8, maxv - maxv // 8, (3, h, w, 3)).astype(dtype)
    xs, ys = _edge_values(w), _edge_values(h)
    X, Y = np.meshgrid(np.array(xs, np.int64), np.array(ys, np.int64))
    pos1 = np.stack([X, Y], axis=2).astype(np.int32)
    pos4 = np.tile(pos1, (1, 4, 1))
    for v in (INT_MIN, INT_MAX):
        assert (pos1[..., 0] == v).any() and (pos1[..., 1] == v).any()
    assert ((pos1 & 31) == 31).any(axis=(0, 1)).all() and ((pos1 & 31) == 0).any(axis=(0, 1)).all()
    assert (~L.taps_inside(pos1, w, h)).mean() > 0.5
    sx, sy = pos1[..., 0].astype(np.int64) >> 5, pos1[..., 1].astype(np.int64) >> 5
    all_out = (sx + 1 < 0) | (sx > w - 1) | (sy + 1 < 0) | (sy > h - 1)
    assert all_out.any()
    for pos, aligned in ((pos1, False), (pos4, True)):
        for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
            want = L.remap_batch(src, pos, border, maxv)
            if border == vs.BORDER_CLAMP:
                assert want.min() >= src.min() and want.max() <= src.max()
            else:
                assert not want[:, np.tile(all_out, (1, pos.shape[1] // pos1.shape[1]))].any()
            got = _dev_remap(vs, src, pos, code, border, src_guard=maxv, aligned=aligned)
            assert np.array_equal(got, want), (pos.shape, border, int((got != want).sum()))


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples.  Premises: the blend's saturation is live (the result
    under max_value 65535 differs) and a remapped sample never exceeds the maximum"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((131, 37), (132, 20)):
        src = rng.integers(0, maxv + 1, (2, h, w, 3)).astype(dtype)
        for f in src:
            f[rng.random((h, w)) < 0.08] = 65535
            f[rng.random((h, w, 3)) < 0.05] = maxv + 1
        pos = np.stack([rng.integers(-64, 32 * w + 64, (h, w)), rng.integers(-64, 32 * h + 64, (h, w))], axis=2).astype(np.int32)
        for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
            want = L.remap_batch(src, pos, border, maxv)
            assert not np.array_equal(want, L.remap_batch(src, pos, border, 65535)) and want.max() == maxv
            got = _dev_remap(vs, src, pos, code, border, src_guard=7, aligned=w % 4 == 0)
            assert np.array_equal(got, want), (w, h, border, int((got != want).sum()))


def test_a_lens_whose_denominator_vanishes_on_a_ring(gpu_vs):
    """1 + k4 r2 passes through 0 on a ring inside the frame: positions there run through the whole int range and saturate.  The device map
    equals the restatement, and the remap through it is defined everywhere.  Premises: the map holds positions far outside the frame on both
    sides and jumps of more than the frame between neighbours"""
    import torch
    vs = gpu_vs
    w, h = 96, 64
    kw = dict(COEFFS["pole"], k4=-4.0, fx=64.0, fy=64.0, cx=48.0, cy=32.0)         # r2 == 0.25, the denominator exactly 0, at (48 +- 32, 32) and (48, 32 +- 32)
    want = L.lens_map(L.params(w, h, **kw), w, h)
    # there kr is an infinity: x * kr saturates with x's sign, y * kr = 0 * infinity is NaN -> 0
    assert tuple(want[32, 80]) == (INT_MAX, 0) and tuple(want[32, 16]) == (INT_MIN, 0) and tuple(want[0, 48]) == (0, INT_MIN)
    assert (want < -32 * 10000).any() and (want > 32 * 10000).any()
    assert (np.abs(np.diff(want[..., 0], axis=1)) > 32 * w).any()
    dev = torch.zeros((h, w, 2), dtype=torch.int32, device="cuda")
    vs.lens_map_device(vs.lens_params(w, h, **kw), w, h, dev.data_ptr())
    torch.cuda.synchronize()
    pos = dev.cpu().numpy()
    assert np.array_equal(pos, want)
    rng = np.random.default_rng(1)
    src = rng.integers(30, 220, (2, h, w, 3)).astype(np.uint8)
    for border in (vs.BORDER_CLAMP, vs.BORDER_CONSTANT):
        got = _dev_remap(vs, src, pos, vs.FMT_BGR8, border, src_guard=255, aligned=True)
        assert np.array_equal(got, L.remap_batch(src, pos, border, 255)), border


CHILD = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
import numpy as np
from video_stabilizer_amd import capi as G, synth
dig = hashlib.sha256()
rng = np.random.default_rng(5)
for dtype, maxv, fmt, (w, h) in ((np.uint8, 255, G.FMT_BGR8, (260, 33)), (np.uint16, 1023, G.FMT_BGR10, (129, 65)), (np.uint8, 255, G.FMT_BGR8, (2, 1))):
    img = rng.integers(0, maxv + 1, (3, h, w, 3)).astype(dtype)
    pos = np.stack([rng.integers(-96, 32 * w + 96, (h, w)), rng.integers(-96, 32 * h + 96, (h, w))], axis=2).astype(np.int32)
    for border in (G.BORDER_CLAMP, G.BORDER_CONSTANT):
        for kw in (dict(), dict(src_stride=3 * w + 7, dst_stride=3 * w + 5, map_stride=2 * w + 3)):
            dig.update(G.remap_batch(img, pos, border=border, fmt=fmt, **kw).tobytes())
clip = np.maximum(synth.make_clip(96, 64, 14, seed=5, channels=3)[0], 1)
lens = G.lens_params(96, 64, k1=-0.2, k2=0.05, p1=0.001, p2=-0.002, zoom=1.05)
dig.update(G.lens_map(lens, 96, 64).tobytes())
for kw in (dict(crop_pixels=8), dict(crop_pixels=0, border_fill=3, denoise=2, inpaint=1)):
    kw = dict(dict(device=0, lag=4, lens=(lens, 96, 64), pyramid_min_width=10, pyramid_min_height=10), **kw)
    s = G.Stabilizer(**kw)
    for fr in clip:
        o = s.process(fr)
        dig.update(b"-" if o is None else o.tobytes())
    out, has = G.Stabilizer(**kw).process_batch(clip)
    dig.update(repr(has).encode() + out[np.array(has, bool)].tobytes())
print("DIGEST", dig.hexdigest())
"""


def test_the_lens_pass_does_not_depend_on_what_fresh_allocations_contain(gpu_vs):
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
    """every allocation of a process_batch call with the pass on is failed once (vs_test_fail_alloc) -- the map, the staged span and the
    corrected batch among them: the call reports it, the next call on the handle equals a fresh handle's"""
    vs = gpu_vs
    from video_stabilizer_amd import synth
    frames = np.maximum(synth.make_clip(96, 64, 12, seed=7, channels=3, bits=8)[0], 1)
    lens = vs.lens_params(96, 64, k1=-0.2, k2=0.05, zoom=1.05)

    def call(s):
        out, has = s.process_batch(frames)
        return list(has), out.tobytes()
    kw = dict(device=0, lag=4, smoother_memory=2, crop_pixels=8, pyramid_min_width=10, pyramid_min_height=10)

    def allocations(make):
        h = make()
        vs.test_fail_alloc(1 << 30)
        call(h)
        return vs.test_fail_alloc(0)
    allocations(lambda: vs.Stabilizer(**kw))                         # (the process-wide staging pool fills on the first call)
    n_off, n_on = allocations(lambda: vs.Stabilizer(**kw)), allocations(lambda: vs.Stabilizer(lens=(lens, 96, 64), **kw))
    assert n_on == n_off + 2                                         # the map and the staged span join the protocol (batch_in is there either way)
    fired = walk(vs, lambda: vs.Stabilizer(lens=(lens, 96, 64), **kw), call, n_on, throwing)
    assert fired == n_on


@pytest.mark.parametrize("throwing", [False, True])
def test_remap_batch_survives_every_allocation_failure(gpu_vs, throwing):
    """the kernel-level call on host memory (frames, map and output are staged): every allocation failed once"""
    vs = gpu_vs
    rng = np.random.default_rng(9)
    # (a size no other test stages: the walk starts from an empty spot of the staging pool or from a warm one, and ends either way)
    src = rng.integers(0, 256, (3, 37, 211, 3)).astype(np.uint8)
    pos = np.stack([rng.integers(-96, 32 * 211 + 96, (41, 200)), rng.integers(-96, 32 * 37 + 96, (41, 200))], axis=2).astype(np.int32)
    want = L.remap_batch(src, pos, vs.BORDER_CLAMP, 255)

    def call(_):
        return vs.remap_batch(src, pos).tobytes()
    assert call(None) == want.tobytes()
    walk(vs, lambda: None, call, 0, throwing)
