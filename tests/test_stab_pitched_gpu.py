"""Pitched frames into the stabilizer.  vs_stabilizer_process_batch / _clips take frames with a row stride and a frame stride of the caller's
choosing, from host or device memory; inside, the frames are made dense on the device (vs_stabilizer.hip, make_dense): pitched host frames
travel as one linear copy of their span and are made dense by 2-D copies on the device, in one call or chunk by chunk through the uploader
thread; pitched device frames are 2-D copies.  None of that may change a byte: the same frames embedded in a buffer of random bytes -- rows of
966 elements (no multiple of 4) 3*w + 5 apart, frames h*stride + 3 apart, starting 1 element in -- give the outputs, the has_output flags and the
accumulated transform of the dense run, bit for bit; a pitched OUTPUT (frames ow*oh*3 + 7 apart) leaves the gaps alone, and the input buffer
is only read.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N, LAG, CROP = 322, 242, 14, 3, 8
OW, OH = W - 2 * CROP, H - 2 * CROP
KW = dict(lag=LAG, smoother_memory=2, crop_pixels=CROP)
STRIDE = 3 * W + 5                    # elements
FSTRIDE = H * STRIDE + 3
START = 1
OUT_GAP = 7
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dense_runs(gpu_vs):
    """(frames, outputs, has_output, accum) of the dense process_batch / process_clips on a fresh handle, per (bits, clips); computed once"""
    from video_stabilizer_amd import synth
    memo = {}

    def get(bits, clips):
        if (bits, clips) not in memo:
            frames, _ = synth.make_clip(W, H, N, seed=91, channels=3, bits=bits)
            st = gpu_vs.Stabilizer(device=0, **KW)
            out, has = st.process_clips(frames, clips) if clips else st.process_batch(frames)
            _, accum, ok = st.state()
            if not clips:                 # (process_clips ends with a reset: nothing to read)
                assert ok, "the dense run must end on a successful alignment: else two failure paths are compared"
            per_clip = N // clips if clips else N
            assert sum(has) == max(clips, 1) * (per_clip - LAG)
            for a in (frames, out):
                a.setflags(write=False)
            memo[(bits, clips)] = (frames, out, has, accum.tup())
        return memo[(bits, clips)]
    return get


def _embed(frames, rng):
    """the frames inside a buffer of random bytes: returns (buffer, view of the frames in it)"""
    dt = frames.dtype
    buf = rng.integers(0, 256 if dt == np.uint8 else 1024, START + N * FSTRIDE, dtype=dt)
    for i in range(N):
        rows = buf[START + i * FSTRIDE:][:H * STRIDE].reshape(H, STRIDE)
        rows[:, :3 * W] = frames[i].reshape(H, 3 * W)
    return buf


@pytest.mark.parametrize("bits,mem,chunked,clips,out_gap", [
    (8, "host", False, 0, 0), (10, "host", False, 0, OUT_GAP),
    (8, "host", True, 0, OUT_GAP), (10, "host", True, 0, 0),
    (8, "device", False, 0, 0), (10, "device", False, 0, OUT_GAP),
    (8, "host", True, 2, OUT_GAP),
])
def test_pitched_frames_give_the_dense_run_bit_for_bit(gpu_vs, dense_runs, monkeypatch, bits, mem, chunked, clips, out_gap):
    import torch
    frames, want, want_has, want_accum = dense_runs(bits, clips)
    dt = frames.dtype
    esz = dt.itemsize
    buf = _embed(frames, np.random.default_rng(7))
    before = buf.copy()
    ofs = OW * OH * 3 + out_gap                                    # output frame stride, elements
    sent = np.array(SENTINEL | (SENTINEL << 8 if esz == 2 else 0), dt)
    out = np.full(N * ofs, sent, dt)
    if chunked:                                                     # five dense frames: chunks of 5, 5, 4 (clip mode: whole clips, 7 and 7)
        monkeypatch.setenv("VS_INGEST_CHUNK_BYTES", str(W * H * 3 * esz * 5))
    else:
        monkeypatch.delenv("VS_INGEST_CHUNK_BYTES", raising=False)
    st = gpu_vs.Stabilizer(device=0, **KW)
    has = (C.c_int32 * N)()
    ow, oh = C.c_int(), C.c_int()
    fmt = gpu_vs.FMT_BGR8 if bits == 8 else gpu_vs.FMT_BGR10
    if mem == "device":
        tdt = torch.uint8 if esz == 1 else torch.int16              # int16 carries the u16 bit pattern
        dbuf = torch.from_numpy(buf.view(np.uint8 if esz == 1 else np.int16)).cuda()
        dout = torch.from_numpy(out.view(np.uint8 if esz == 1 else np.int16)).cuda()
        assert dbuf.dtype == tdt
        src, dst, where = dbuf.data_ptr() + START * esz, dout.data_ptr(), gpu_vs.MEM_DEVICE
    else:
        src, dst, where = buf.ctypes.data + START * esz, out.ctypes.data, gpu_vs.MEM_HOST
    L = gpu_vs.lib()
    if clips:
        r = L.vs_stabilizer_process_clips(st.h, C.c_void_p(src), FSTRIDE, clips, N // clips, W, H, STRIDE, fmt, where, C.c_void_p(dst), ofs,
                                          has, C.byref(ow), C.byref(oh))
    else:
        r = L.vs_stabilizer_process_batch(st.h, C.c_void_p(src), FSTRIDE, N, W, H, STRIDE, fmt, where, C.c_void_p(dst), ofs, has,
                                          C.byref(ow), C.byref(oh))
    assert r >= 0, L.vs_last_error().decode()
    if mem == "device":
        torch.cuda.synchronize()
        out = dout.cpu().numpy().view(dt)
        buf = dbuf.cpu().numpy().view(dt)
    per_clip = N // clips if clips else N
    assert (ow.value, oh.value) == (OW, OH)
    assert list(has) == want_has and r == sum(want_has)
    for c in range(max(clips, 1)):
        assert sum(has[c * per_clip:(c + 1) * per_clip]) == per_clip - LAG
    got = out.reshape(N, ofs)
    for i in range(N):
        if has[i]:
            assert np.array_equal(got[i, :OW * OH * 3], want[i].reshape(-1)), "output frame %d" % i
        else:
            assert (got[i, :OW * OH * 3] == sent).all(), "frame %d has no output and was written" % i
    if out_gap:
        assert (got[:, OW * OH * 3:] == sent).all(), "the gap between output frames was written"
    assert np.array_equal(buf, before), "the input buffer was written"
    if not clips:
        assert st.state()[1].tup() == want_accum
