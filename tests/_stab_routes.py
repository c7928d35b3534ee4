"""How the stabilizer tests drive a handle and compare what comes out: the routes (frame by frame, host batches, device memory), and the
allocation-failure walk.  `vs` is the product's C ABI (video_stabilizer_amd.capi), `st` a vs.Stabilizer.  Outputs are {k: output frame k}.

Test infrastructure only.
"""
import gc

import numpy as np


def frame_by_frame(st, frames, states=None):
    """process() frame by frame; states: a list that gets (measured, accumulated, success, has output) after every frame"""
    out = {}
    for i, f in enumerate(frames):
        o = st.process(f)
        if states is not None:
            m, a, s = st.state()
            states.append((m.tup(), a.tup(), s, o is not None))
        if o is not None:
            out[i - st.params.lag] = o
    return out


def batches(st, frames, sizes, fmt=None):
    """process_batch() calls of the sizes given, over and over until the clip ends"""
    out, i, k = {}, 0, 0
    while i < len(frames):
        m = min(sizes[k % len(sizes)], len(frames) - i)
        o, has = st.process_batch(frames[i:i + m], fmt=fmt)
        for j in range(m):
            if has[j]:
                out[i + j - st.params.lag] = o[j].copy()
        i, k = i + m, k + 1
    return out


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def device_batch(vs, st, frames, fmt=None):
    """the device-memory route: upload, process_batch_device, synchronize, read back -> ({k: frame}, the call's count of output frames).
    fmt: uint16 frames are 10-bit unless the caller says otherwise"""
    import torch
    n, h, w, _ = frames.shape
    if fmt is None:
        fmt = vs.FMT_BGR8 if frames.dtype == np.uint8 else vs.FMT_BGR10
    ow, oh = st.delivered_size(w, h)
    dev = torch.from_numpy(frames if frames.dtype == np.uint8 else frames.view(np.int16)).cuda()
    dout = torch.zeros((n, oh, ow, 3), dtype=dev.dtype, device="cuda")
    r, has = st.process_batch_device(dev.data_ptr(), n, w, h, fmt, dout.data_ptr())
    torch.cuda.synchronize()
    res = dout.cpu().numpy().view(frames.dtype)
    return {i - st.params.lag: res[i] for i, hh in enumerate(has) if hh}, r


def assert_every_route_equals(vs, kw, frames, ref, sizes):
    """process_batch (one call; split calls of `sizes`, which add up to the clip) and device memory, each on a fresh vs.Stabilizer(**kw),
    against ref = frame_by_frame's outputs, bit for bit"""
    lag = kw["lag"]
    out, has = vs.Stabilizer(**kw).process_batch(frames)
    assert [i - lag for i, hh in enumerate(has) if hh] == sorted(ref)
    for i, hh in enumerate(has):
        if hh:
            assert np.array_equal(out[i], ref[i - lag]), ("one call", i)
    # split calls: queued frames become buffers of the handle between the calls and are candidates of the next call's jobs
    st = vs.Stabilizer(**kw)
    pos = 0
    for m in sizes:
        o, hs = st.process_batch(frames[pos:pos + m])
        for i, hh in enumerate(hs):
            if hh:
                assert np.array_equal(o[i], ref[pos + i - lag]), ("split calls", pos, i)
        pos += m
    assert pos == len(frames)
    # device-resident frames
    res, r = device_batch(vs, vs.Stabilizer(**kw), frames)
    assert r == len(ref) and sorted(res) == sorted(ref)
    for k in sorted(res):
        assert np.array_equal(res[k], ref[k]), ("device memory", k + lag)


def walk(vs, make, call, min_fired, throwing=False, stride=1):
    """the allocation-failure protocol (tests/test_alloc_failure_gpu.py): every allocation of call(make()) is failed once; the call reports it,
    the next call on the handle equals a fresh handle's, the handle keeps working.  Returns the number of allocations that were failed.
    throwing: the allocation THROWS std::bad_alloc instead (vs_test_fail_alloc(-k)) -- a host allocation failing at that point of the call: the
    exception must stop at the C boundary (VS_ERR_NOMEM = -5) and leave the handle exactly as an error code does; stride: every stride-th k only"""
    vs.test_fail_alloc(0)
    call(make())                                   # process-wide one-time allocations (the warp's parameter ring) happen here
    ref = call(make())
    fired, k = 0, 1
    while True:
        h = make()
        vs.test_fail_alloc(-k if throwing else k)
        try:
            got, failed = call(h), False
        except vs.VsError as e:
            failed = True
            if throwing:
                assert "error -5" in str(e) and "bad_alloc" in str(e), str(e)
            else:
                assert "error -2" in str(e) and "out of memory" in str(e).lower(), str(e)
        seen = vs.test_fail_alloc(0)
        if not failed:
            assert seen < k, "allocation %d was failed (of %d made) but the call reported success" % (k, seen)
            assert got == ref
            break
        assert seen >= k
        fired += 1
        assert call(h) == ref, "k = %d: the call after the failed one differs from a fresh handle" % k
        assert call(h) is not None                 # and the handle keeps working (state carried over from a good call)
        del h
        gc.collect()
        k += stride
        assert k < 400, "the walk does not terminate"
    assert fired >= min_fired, "only %d allocations were failed: the hook does not see the call's allocations" % fired
    return fired
