"""The aligner's chunk machinery (vs_engine.hip: chunk_begin / chunk_end, ensure_capacity, the three ways align_start cuts a batch) on the
routes the other suites leave out: a device-resident batch longer than the 1024-frame chunk (the base pointer of the second chunk, the
carry-over between chunks), device-resident clips that fill more than one chunk, and a handle whose storage grows in the middle of a
sequence.  Every result is compared bit for bit -- status and transform -- with the same frames fed one at a time (or clip by clip)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N, CLIP = 64, 48, 1030, 10
PYR = dict(pyramid_min_width=16, pyramid_min_height=12)


def _bits(status, ts):
    return [int(s) for s in status], [bytes(t) for t in ts]


def _same(got, want, can_pair):
    """can_pair: the frames that have a predecessor in their sequence"""
    gs, gt = _bits(*got)
    ws, wt = _bits(*want)
    assert gs == ws
    bad = [i for i in range(len(wt)) if gt[i] != wt[i]]
    assert not bad, "transforms differ at frames %s" % bad[:8]
    assert sum(ws) > 0.9 * can_pair, (sum(ws), can_pair)       # (the comparison is about solved pairs, not a row of failures)


@pytest.fixture(scope="module")
def frames10():
    """1030 small 10-bit BGR frames: jitter without a pan, so the camera stays inside the texture's margin"""
    from video_stabilizer_amd import synth
    frames, _ = synth.make_clip(W, H, N, seed=41, channels=3, bits=10, pan=0.0, jitter_t=1.5)
    return frames


def _to_device(arr_u16):
    import torch
    return torch.from_numpy(arr_u16.view(np.int16)).cuda()     # int16 carries the u16 bit pattern


def test_device_batch_past_the_chunk_bound_equals_frame_by_frame(gpu_vs, frames10):
    vs = gpu_vs
    stride = W * 3 + 6
    fs = H * stride + 10
    pitched = np.full(N * fs, 0x3ff, np.uint16)                # (the padding holds valid but foreign pixels)
    rows = np.lib.stride_tricks.as_strided(pitched, (N, H, W * 3), (fs * 2, stride * 2, 2))
    rows[:] = frames10.reshape(N, H, W * 3)
    dev = _to_device(pitched)
    got = vs.Aligner(device=0, **PYR).align_batch_device(dev.data_ptr(), N, W, H, vs.FMT_BGR10, stride=stride, frame_stride=fs)
    one = vs.Aligner(device=0, **PYR)
    want = [one.align_next(f) for f in frames10]
    _same(got, ([int(ok) for ok, _ in want], [t for _, t in want]), N - 1)


def test_device_clips_over_two_chunks_equal_clip_by_clip(gpu_vs, frames10):
    vs = gpu_vs
    dev = _to_device(np.ascontiguousarray(frames10).reshape(-1))
    got = vs.Aligner(device=0, **PYR).align_clips(N, N // CLIP, mem_ptr=dev.data_ptr(), w=W, h=H, fmt=vs.FMT_BGR10)
    one = vs.Aligner(device=0, **PYR)
    status, ts = [], []
    for c in range(N // CLIP):
        one.reset()
        s, t = one.align_batch(frames10[c * CLIP:(c + 1) * CLIP])
        status += s
        ts += t
    _same(got, (status, ts), N - N // CLIP)
    assert [i for i, s in enumerate(status) if i % CLIP == 0 and s] == []      # every clip starts a sequence of its own


@pytest.mark.parametrize("mode", ["SELECT_DEVICE", "SELECT_STL_HOST"])
def test_growth_in_mid_sequence_carries_the_last_frame_over(gpu_vs, mode):
    vs = gpu_vs
    from video_stabilizer_amd import synth
    frames, _ = synth.make_clip(320, 240, 19, seed=43, channels=3)
    a = vs.Aligner(device=0, select_mode=getattr(vs, mode))
    status, ts = [], []

    def take(res):
        status.extend(int(s) for s in res[0])
        ts.extend(res[1])

    for f in frames[0:3]:
        ok, t = a.align_next(f)
        take(([ok], [t]))
    take(a.align_batch(frames[3:8]))                           # the storage grows; frame 2 moves to the new slabs
    for f in frames[8:10]:
        ok, t = a.align_next(f)
        take(([ok], [t]))
    take(a.align_batch(frames[10:19]))                         # ... and again
    one = vs.Aligner(device=0, select_mode=getattr(vs, mode))
    want = [one.align_next(f) for f in frames]
    _same((status, ts), ([int(ok) for ok, _ in want], [t for _, t in want]), len(frames) - 1)
