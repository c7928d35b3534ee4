"""The aligner's resident state, byte for byte: the gray pyramid of EVERY frame of a call and the keypoint / Jacobian tables of every keyframe
equal the oracle's stage functions (tests/_align_state.py: reference_state) -- through batches on the 4-row and the 16-row build of
vs_k_pyr_down_rows, second calls that start on a keyframe, clip calls, every route of vs_k_ingest_pyr (byte loop, group loads with rim tiles
only / interior tiles / one tile column, widths that are no multiple of 4 on padded pitches, base offsets, routes that change between the frames
of one launch, host and device memory), the four BGR depths on colours at the gray formula's rounding boundary, and the one-launch keyframe
kernel at all ten tile sizes on hostile content.  No tolerances: every comparison is equality of bytes (tests/test_align_state_cpu.py proves the
inputs and that the comparison can fail)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_state as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _noise(w, h, fmt, seed, tiny):
    """a noise frame and its reference state, computed once"""
    f = _freeze(S.noise(w, h, seed, fmt))
    return f, S.reference_state(f, fmt, **(S.TINY if tiny else {}))


@functools.lru_cache(maxsize=None)
def _hostile(w, h, kind, seed):
    f = _freeze(S.keyframe_hostile(w, h, kind, seed))
    return f, S.reference_state(f, O.FMT_GRAY8)


def _call(vs, al, ptr, mem, fmt, n, w, h, pitch, frame_pitch, clips=0):
    """vs_aligner_align_batch / _clips on raw memory: pitches in elements"""
    out, st = (vs.Transform * n)(), (C.c_int32 * n)()
    if clips:
        r = vs.lib().vs_aligner_align_clips(al.h, C.c_void_p(ptr), frame_pitch, clips, n // clips, w, h, pitch, fmt, mem, C.byref(al.params), out, st)
    else:
        r = vs.lib().vs_aligner_align_batch(al.h, C.c_void_p(ptr), frame_pitch, n, w, h, pitch, fmt, mem, C.byref(al.params), out, st)
    assert r >= 0, vs.lib().vs_last_error()


def _dense_call(vs, al, frames, fmt, clips=0):
    frames = np.ascontiguousarray(frames)
    n, h, w = frames.shape[:3]
    pitch = w * S.fmt_channels(fmt)
    _call(vs, al, frames.ctypes.data, vs.MEM_HOST, fmt, n, w, h, pitch, h * pitch, clips)


def _check(al, want, keyframes):
    got = [S.engine_state(al, i, i in keyframes) for i in range(len(want))]
    bad = S.call_diffs(got, want, keyframes)
    assert bad == [], "\n".join(bad[:12])


# ---- every frame of a batch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", S.BATCH_CALLS, ids=[c[0] for c in S.BATCH_CALLS])
@pytest.mark.parametrize("fmt", S.BATCH_FORMATS, ids=["bgr8", "bgr10", "gray8"])
@pytest.mark.parametrize("w,h", S.BATCH_SIZES)
def test_every_frame_of_a_call(gpu_vs, w, h, fmt, call):
    """frames 1 .. n-1 (blockIdx.y, the frame strides, the keyframe runs that step by two frames), calls of 1 and 3 frames on the 4-row
    bands and of 6 on the 16-row bands, a second call whose first frame is a keyframe, clips of odd and of even length"""
    _, clips, ns = call
    pool = [_noise(w, h, fmt, 100 + k, True) for k in range(sum(ns))]
    al = gpu_vs.Aligner(device=0, **S.TINY)
    seen = 0
    for n in ns:
        part = pool[seen:seen + n]
        _dense_call(gpu_vs, al, np.stack([f for f, _ in part]), fmt, clips)
        _check(al, [ref for _, ref in part], S.key_frames(n, seq0=seen, clip_len=n // clips if clips else 0))
        seen += n


# ---- routes of the ingest ----------------------------------------------------------------------------------------------------------------------
def _to_device(buf):
    import torch
    t = torch.from_numpy(buf.view(np.int16) if buf.dtype == np.uint16 else buf).cuda()      # (int16 carries the u16 bit pattern)
    torch.cuda.synchronize()
    assert t.data_ptr() % 256 == 0
    return t


def _run_embedded(vs, al, frames, fmt, pitch, frame_pitch, base_off, device):
    """the frames inside a buffer full of 0xFF; afterwards the buffer is what it was"""
    n, h, w = frames.shape[:3]
    buf, off = S.embed(frames, pitch, frame_pitch, base_off, 0xFF if frames.dtype == np.uint8 else 0xFFFF)
    before = buf.copy()
    es = buf.dtype.itemsize
    if device:
        t = _to_device(buf)
        _call(vs, al, t.data_ptr() + off * es, vs.MEM_DEVICE, fmt, n, w, h, pitch, frame_pitch)
        after = t.cpu().numpy().view(buf.dtype)
    else:
        _call(vs, al, buf.ctypes.data + off * es, vs.MEM_HOST, fmt, n, w, h, pitch, frame_pitch)
        after = buf
    assert np.array_equal(after, before), "the call wrote into its input"


def _route_id(c):
    return "%s-%dx%d-n%d-p%s-f%s-o%d" % ({O.FMT_BGR8: "bgr8", O.FMT_BGR10: "bgr10"}[c[0]], c[1], c[2], c[3], c[4], c[5], c[6])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", S.ROUTE_CASES, ids=[_route_id(c) for c in S.ROUTE_CASES])
def test_ingest_routes(gpu_vs, case, device):
    fmt, w, h, n = case[:4]
    pitch, frame_pitch, base_off = S.route_case_layout(case)
    pool = [_noise(w, h, fmt, 200 + k, True) for k in range(n)]
    al = gpu_vs.Aligner(device=0, **S.TINY)
    _run_embedded(gpu_vs, al, np.stack([f for f, _ in pool]), fmt, pitch, frame_pitch, base_off, device)
    _check(al, [ref for _, ref in pool], S.key_frames(n))


# ---- formats and boundary colours ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _palette_frames(bits, w, h):
    fmt = S.FMT_OF_BITS[bits]
    hi = (1 << bits) - 1
    frames = [S.palette_frame(w, h, bits, 7), np.zeros((h, w, 3), S.fmt_dtype(fmt)), np.full((h, w, 3), hi, S.fmt_dtype(fmt)),
              S.palette_frame(w, h, bits, 8)]
    frames = _freeze(np.stack(frames))
    return frames, [S.reference_state(f, fmt, **S.TINY) for f in frames]


@pytest.mark.parametrize("bits,w,h,pitch", S.palette_cases())
def test_formats_on_boundary_colours(gpu_vs, bits, w, h, pitch):
    """8, 10, 12 and full-range 16 bits on the colours that sit on the gray formula's rounding boundary, the all-zero and the all-max frame and
    (10 and 12 bits) values above the format's maximum, on the group route and in the byte loop"""
    fmt = S.FMT_OF_BITS[bits]
    frames, want = _palette_frames(bits, w, h)
    if 8 < bits < 16:
        assert int(frames.max()) == 0xFFFF and want[0][0]["img"].max() == 255
    assert want[1][0]["img"].max() == 0 and want[2][0]["img"].min() == 255
    pitch = pitch or w * 3
    al = gpu_vs.Aligner(device=0, **S.TINY)
    _run_embedded(gpu_vs, al, frames, fmt, pitch, h * pitch + 4, 0, device=False)
    _check(al, want, S.key_frames(4))


# ---- keyframe tables, every tile size ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", S.KEYFRAME_CALLS, ids=["-".join(k) for k in S.KEYFRAME_CALLS])
@pytest.mark.parametrize("w,h", S.KEYFRAME_SIZES)
def test_keyframe_tables_at_every_tile_size(gpu_vs, w, h, kinds):
    """the engine's route through vs_k_keyframe_levels (tile size changing from level to level inside one launch, offsets from the pyramid
    slot): two keyframes of different kinds in one call, so that a table written to the wrong frame shows"""
    frames = [_noise(w, h, O.FMT_GRAY8, 300, False), _hostile(w, h, kinds[0], 11), _noise(w, h, O.FMT_GRAY8, 301, False), _hostile(w, h, kinds[1], 12)]
    assert frames[1][1][0]["ts"] == S.level_dims(w, h)[0][2]
    al = gpu_vs.Aligner(device=0)
    _dense_call(gpu_vs, al, np.stack([f for f, _ in frames]), O.FMT_GRAY8)
    _check(al, [ref for _, ref in frames], [1, 3])


# ---- nothing read that was never written --------------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np, torch
from video_stabilizer_amd import capi as G
import _align_state as S
import test_align_state_gpu as T
from oracle import oracle as O
assert G.device_count() >= 1
def run(w, h, fmt, n, clips, params):
    frames = [S.noise(w, h, 400 + k, fmt) for k in range(n)]
    want = [S.reference_state(f, fmt, **params) for f in frames]
    al = G.Aligner(device=0, **params)
    T._dense_call(G, al, np.stack(frames), fmt, clips)
    T._check(al, want, S.key_frames(n, clip_len=n // clips if clips else 0))
run(499, 131, O.FMT_BGR8, 6, 0, S.TINY)          # 16-row bands, w %% 4 = 3
run(203, 191, O.FMT_GRAY8, 4, 0, {})
run(129, 33, O.FMT_BGR10, 6, 2, S.TINY)          # two clips of three
print("STATE-OK")
"""


@pytest.mark.parametrize("poison", [165, 90])
def test_state_does_not_depend_on_what_fresh_allocations_contain(gpu_vs, poison):
    """every fresh device allocation of the child starts filled with the poison byte (VS_TEST_POISON_ALLOC, the hook of
    test_uninitialised_memory_gpu.py): a pyramid byte or a table entry the kernels skip reads as the poison"""
    env = dict(os.environ, VS_TEST_HOOKS="1", VS_TEST_POISON_ALLOC=str(poison))
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "STATE-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
