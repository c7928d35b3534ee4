"""The YCbCr conversions (vs_ycbcr.hip) on hostile input, bit for bit against the rule's restatement (tests/_ycbcr_ref.py): frames constant at
every extreme of the container, odd frames whose edge cells must clamp, poisoned allocations, every allocation of the three new calls failed
once.

The kernel-level calls work on DEVICE memory; every plane and the BGR side sit inside guard bands on all four sides, as
tests/test_lens_hostile_gpu.py::_banded lays them out.  Inputs are verified to be only read, destinations to be untouched outside their rows' own
samples.  A source's guard holds a value no frame holds, so an edge cell that reads past column w - 1 or row h - 1 shows in the result: each
such case first asserts, on the restatement, that the clamped edge differs from what the stray read would give."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _ycbcr_ref as R
from _stab_routes import walk
from test_lens_hostile_gpu import G, _banded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ["bgr8", "bgr10", "bgr12"]


class _Dev:
    """one banded plane in device memory: frames (n, rows, row_elems) of `a` inside guard rows and guard padding"""

    def __init__(self, a, stride, guard, lead):
        import torch
        self.n, self.rows, self.row = a.shape
        self.stride, self.guard, self.lead, self.dtype = stride, guard, lead, a.dtype
        self.host = _banded(a, self.row, stride, guard, lead)
        self.dev = torch.from_numpy(self.host.view(np.int16) if a.dtype == np.uint16 else self.host).cuda()
        self.fs = (self.rows + 2 * G) * stride

    def ptr(self, elem=0):
        return self.dev.data_ptr() + (self.lead + G * self.stride + elem) * self.dtype.itemsize

    def back(self):
        return self.dev.cpu().numpy().view(self.dtype).copy()

    def unchanged(self):
        return np.array_equal(self.back(), self.host)

    def result(self):
        """the rows' own samples (n, rows, row_elems); asserts that nothing else was written"""
        b = self.back()
        fr = b[self.lead:self.lead + self.n * (self.rows + 2 * G) * self.stride].reshape(self.n, self.rows + 2 * G, self.stride)
        res = fr[:, G:G + self.rows, :self.row].copy()
        fr[:, G:G + self.rows, :self.row] = self.guard
        assert (b == self.guard).all(), "a destination was written outside its rows' own samples"
        return res


def _plane_set(y, cb, cr, inter, aligned, guard):
    """the banded device planes of (y, cb, cr) and their descriptor fields: ([_Dev, ..], y, cb, cr addresses, y_stride, c_stride, c_step, y_fs, c_fs)"""
    n, h, w = y.shape
    lead = 4 if aligned else 1
    ys = (w + 8) & ~3 if aligned else (w + 3) | 1
    dy = _Dev(y, ys, guard, lead)
    if cb is None:
        return [dy], dy.ptr(), None, None, ys, 0, 1, dy.fs, 0
    ch, cw = cb.shape[1:]
    if inter:
        pairs = np.zeros((n, ch, 2 * cw), y.dtype)
        pairs[:, :, 0::2], pairs[:, :, 1::2] = (cb, cr) if inter == "nv12" else (cr, cb)
        cs = (2 * cw + 8) & ~3 if aligned else (2 * cw + 5) | 1
        dc = _Dev(pairs, cs, guard, lead)
        pa, pb = (dc.ptr(0), dc.ptr(1)) if inter == "nv12" else (dc.ptr(1), dc.ptr(0))
        return [dy, dc], dy.ptr(), pa, pb, ys, cs, 2, dy.fs, dc.fs
    cs = (cw + 8) & ~3 if aligned else (cw + 5) | 1
    du, dv = _Dev(cb, cs, guard, lead), _Dev(cr, cs, guard, lead)
    return [dy, du, dv], dy.ptr(), du.ptr(), dv.ptr(), ys, cs, 1, dy.fs, du.fs


def _split(devs, inter, mono):
    """the (y, cb, cr) a destination plane set holds"""
    y = devs[0].result()
    if mono:
        return y, None, None
    if inter:
        p = devs[1].result()
        a, b = p[:, :, 0::2], p[:, :, 1::2]
        return (y, a, b) if inter == "nv12" else (y, b, a)
    return y, devs[1].result(), devs[2].result()


def _dev_to_bgr(vs, code, y, cb, cr, sub, inter, aligned, src_guard):
    import torch
    n, h, w = y.shape
    dguard = 0x5A if y.dtype.itemsize == 1 else 0x5A5A
    devs, py, pcb, pcr, ys, cs, step, yfs, cfs = _plane_set(y, cb, cr, inter, aligned, src_guard)
    bs = (3 * w + 8) & ~3 if aligned else (3 * w + 7) | 1
    dst = _Dev(np.full((n, h, 3 * w), dguard, y.dtype), bs, dguard, 4 if aligned else 1)
    torch.cuda.synchronize()
    vs.ycbcr_to_bgr_batch_device(vs.ycbcr_planes(py, pcb, pcr, ys, cs, step, sub, yfs, cfs), n, w, h, code, dst.ptr(), dst.fs, bs)
    torch.cuda.synchronize()
    assert all(d.unchanged() for d in devs)                                         # inputs are only read
    return dst.result().reshape(n, h, w, 3)


def _dev_to_ycbcr(vs, code, bgr, sub, inter, mono, aligned, src_guard):
    import torch
    n, h, w, _ = bgr.shape
    dguard = 0x5A if bgr.dtype.itemsize == 1 else 0x5A5A
    cw, ch = R.chroma_shape(w, h, sub)
    blank = (lambda *s: np.full(s, dguard, bgr.dtype))
    devs, py, pcb, pcr, ys, cs, step, yfs, cfs = _plane_set(blank(n, h, w), None if mono else blank(n, ch, cw), None if mono else blank(n, ch, cw), inter, aligned, dguard)
    bs = (3 * w + 8) & ~3 if aligned else (3 * w + 7) | 1
    src = _Dev(bgr.reshape(n, h, 3 * w), bs, src_guard, 4 if aligned else 1)
    torch.cuda.synchronize()
    vs.bgr_to_ycbcr_batch_device(src.ptr(), src.fs, n, w, h, bs, code, vs.ycbcr_planes(py, pcb, pcr, ys, cs, step, sub, yfs, cfs))
    torch.cuda.synchronize()
    assert src.unchanged()
    return _split(devs, inter, mono)


def _same(got, want):
    return all((g is None and r is None) or np.array_equal(g, r) for g, r in zip(got, want))


@pytest.mark.parametrize("layout", ["i420", "nv12", "nv21", "i422", "i444", "mono"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_frames_constant_at_every_extreme(gpu_vs, fmt, layout):
    """every plane constant at 0, at the format's maximum and at the container's maximum above it, in every combination per plane; (8, 6) in the
    wide form (buffers on dwords), (7, 5) in the narrow one.  Premises: both clamps fire, and -- towards YCbCr -- samples above the maximum are cut"""
    vs = gpu_vs
    code, dtype, bits = R.FORMATS[fmt]
    sub, inter, mono = R.LAYOUTS[layout]
    maxv, top = (1 << bits) - 1, int(np.iinfo(dtype).max)
    levels = sorted({0, maxv, top})
    seen = set()
    for (w, h), aligned in (((8, 6), True), ((7, 5), False)):
        cw, ch = R.chroma_shape(w, h, sub)
        combos = [(a, b, c) for a in levels for b in levels for c in levels]
        n = len(combos)
        y = np.stack([np.full((h, w), a, dtype) for a, _, _ in combos])
        cb = None if mono else np.stack([np.full((ch, cw), b, dtype) for _, b, _ in combos])
        cr = None if mono else np.stack([np.full((ch, cw), c, dtype) for _, _, c in combos])
        want = R.to_bgr(y, cb, cr, sub, bits)
        seen |= set(np.unique(want).tolist())
        got = _dev_to_bgr(vs, code, y, cb, cr, sub, inter, aligned, src_guard=maxv // 2 + 3)
        assert np.array_equal(got, want), (w, h)
        bgr = np.stack([np.broadcast_to(np.array(c, dtype), (h, w, 3)) for c in combos]).copy()
        wantp = R.to_ycbcr(bgr, sub, bits, mono)
        if top > maxv:
            assert _same(wantp, R.to_ycbcr(np.minimum(bgr, maxv), sub, bits, mono)) and wantp[0].max() <= maxv
        assert n == len(levels) ** 3 and _same(_dev_to_ycbcr(vs, code, bgr, sub, inter, mono, aligned, src_guard=maxv // 2 + 3), wantp), (w, h)
    assert {0, maxv} <= seen


@pytest.mark.parametrize("layout", ["i420", "nv12", "i422"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_cells_clamp_and_do_not_stray(gpu_vs, fmt, layout):
    """odd frames, constant in a saturated colour, towards YCbCr: the last cell of a row holds one real column (and, 4:2:0, the last cell row one
    real row).  The source's padding and guard rows hold mid-gray, which no frame holds: a cell that read them would average towards neutral
    chroma.  (7, 5) and (1, 1) in the narrow form; (12, 5) in the wide form, whose bottom cell row clamps (4:2:0)."""
    vs = gpu_vs
    code, dtype, bits = R.FORMATS[fmt]
    sub, inter, mono = R.LAYOUTS[layout]
    maxv, top = (1 << bits) - 1, int(np.iinfo(dtype).max)
    gray = maxv // 2 + 3
    colours = [(0, maxv, top), (top, 0, maxv), (maxv, top, 0), (0, 0, maxv), (maxv, 0, 0)]
    for (w, h), aligned in (((7, 5), False), ((1, 1), False), ((12, 5), True)):
        if (w % 2 == 0 or sub[0] == 0) and (h % 2 == 0 or sub[1] == 0):
            continue                                                               # (no cell of this layout reaches past the frame)
        bgr = np.stack([np.broadcast_to(np.array(c, dtype), (h, w, 3)) for c in colours]).copy()
        assert not (bgr == gray).any()
        want = R.to_ycbcr(bgr, sub, bits, mono)
        # what a stray read would give: the frame continued by the guard's gray instead of its own edge
        bx, by = 1 << sub[0], 1 << sub[1]
        cw, ch = R.chroma_shape(w, h, sub)
        grown = np.full((len(colours), ch * by, cw * bx, 3), gray, dtype)
        grown[:, :h, :w] = bgr
        stray = R.to_ycbcr(grown, sub, bits, mono)
        assert not np.array_equal(stray[1], want[1]) and not np.array_equal(stray[2], want[2])
        got = _dev_to_ycbcr(vs, code, bgr, sub, inter, mono, aligned, src_guard=gray)
        assert _same(got, want), (w, h)
        # and back: the replicated chroma of the odd edge
        rng = np.random.default_rng(w * 31 + h)
        planes = [rng.integers(0, top + 1, p.shape).astype(dtype) for p in want]
        assert np.array_equal(_dev_to_bgr(vs, code, *planes, sub, inter, aligned, src_guard=gray), R.to_bgr(*planes, sub, bits)), (w, h)


CHILD = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
from video_stabilizer_amd import capi as V, synth
import _ycbcr_ref as R
dig = hashlib.sha256()
rng = np.random.default_rng(11)
for name, (w, h) in (("bgr8", (260, 33)), ("bgr10", (129, 65)), ("bgr8", (2, 1))):
    code, dtype, bits = R.FORMATS[name]
    for layout in ("i420", "nv21", "i444", "mono"):
        sub, inter, mono = R.LAYOUTS[layout]
        cw, ch = R.chroma_shape(w, h, sub)
        top = np.iinfo(dtype).max + 1
        y = rng.integers(0, top, (3, h, w)).astype(dtype)
        cb = None if mono else rng.integers(0, top, (3, ch, cw)).astype(dtype)
        cr = None if mono else rng.integers(0, top, (3, ch, cw)).astype(dtype)
        bgr = V.ycbcr_to_bgr_batch(y, cb, cr, sub=sub, fmt=code, interleaved=inter)
        dig.update(bgr.tobytes())
        for p in V.bgr_to_ycbcr_batch(bgr, sub=sub, fmt=code, interleaved=inter, mono=mono, y_stride=w + 3, src_stride=3 * w + 5):
            dig.update(b"-" if p is None else p.tobytes())
clip = np.maximum(synth.make_clip(96, 64, 14, seed=5, channels=3)[0], 1)
y, cb, cr = R.to_ycbcr(clip, (1, 1), 8)
for kw in (dict(crop_pixels=8), dict(crop_pixels=0, border_fill=3, denoise=2, inpaint=1)):
    kw = dict(dict(device=0, lag=4, pyramid_min_width=10, pyramid_min_height=10), **kw)
    for inter in (None, "nv12"):
        planes, has = V.Stabilizer(**kw).process_batch_ycbcr(y, cb, cr, interleaved=inter)
        dig.update(repr(has).encode())
        for p in planes:
            dig.update(p[np.array(has, bool)].tobytes())
print("DIGEST", dig.hexdigest())
"""


def test_the_conversions_do_not_depend_on_what_fresh_allocations_contain(gpu_vs):
    """one child process per fill byte of every fresh device allocation (VS_TEST_POISON_ALLOC): the three new calls give the same bytes"""
    digests = []
    for byte in (255, 0):
        env = dict(os.environ, VS_TEST_POISON_ALLOC=str(byte), VS_TEST_HOOKS="1")
        out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        digests.append([line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1])
    assert digests[0] == digests[1]


@pytest.mark.parametrize("throwing", [False, True])
def test_the_batch_calls_survive_every_allocation_failure(gpu_vs, throwing):
    """the two kernel-level calls on host memory (every plane and the BGR side are staged): every allocation failed once"""
    vs = gpu_vs
    rng = np.random.default_rng(13)
    # (sizes no other test stages: the walk starts from an empty spot of the staging pool or from a warm one, and ends either way)
    y, cb, cr = (rng.integers(0, 256, s).astype(np.uint8) for s in ((3, 39, 213), (3, 20, 107), (3, 20, 107)))
    want = R.to_bgr(y, cb, cr, (1, 1), 8)
    wantp = R.to_ycbcr(want, (1, 1), 8)

    def to_bgr(_):
        return vs.ycbcr_to_bgr_batch(y, cb, cr).tobytes()

    def to_ycbcr(_):
        return b"".join(p.tobytes() for p in vs.bgr_to_ycbcr_batch(want, interleaved="nv12"))
    assert to_bgr(None) == want.tobytes() and to_ycbcr(None) == b"".join(p.tobytes() for p in wantp)
    walk(vs, lambda: None, to_bgr, 0, throwing)
    walk(vs, lambda: None, to_ycbcr, 0, throwing)


@pytest.mark.parametrize("throwing", [False, True])
def test_process_batch_ycbcr_survives_every_allocation_failure(gpu_vs, throwing):
    """every allocation of a process_batch_ycbcr call on host planes is failed once -- the handle's two BGR buffers and the staged spans among
    them: the call reports it, the next call on the handle equals a fresh handle's"""
    vs = gpu_vs
    from video_stabilizer_amd import synth
    frames = np.maximum(synth.make_clip(96, 64, 12, seed=7, channels=3, bits=8)[0], 1)
    y, cb, cr = R.to_ycbcr(frames, (1, 1), 8)
    kw = dict(device=0, lag=4, smoother_memory=2, crop_pixels=8, pyramid_min_width=10, pyramid_min_height=10)

    def call(s):
        planes, has = s.process_batch_ycbcr(y, cb, cr)
        return list(has), b"".join(p.tobytes() for p in planes)

    def allocations(fn):
        h = vs.Stabilizer(**kw)
        vs.test_fail_alloc(1 << 30)
        fn(h)
        return vs.test_fail_alloc(0)
    allocations(call)                                                              # (the process-wide staging pool fills on the first call)
    n = allocations(call)
    assert n >= 2                                                                  # a fresh handle's two BGR buffers at the least
    fired = walk(vs, lambda: vs.Stabilizer(**kw), call, n, throwing)
    assert fired == n
