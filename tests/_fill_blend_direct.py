"""The fill-blend calls of the C ABI made on DEVICE memory inside guard bands (the host-memory form copies only the rows' own bytes back, and
stages every buffer into a fresh, aligned allocation): the destination windows G rows apart in a guard-filled buffer, the sums between guard
values, the source at any base offset and pitch.  Shared by tests/test_fill_blend_gpu.py and tests/test_fill_blend_hostile_gpu.py."""
import ctypes as C

import numpy as np

G = 3
SUMS_GUARD = 0x5A5A5A5A5A5A5A5A


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _back(t, dtype):
    return t.cpu().numpy().view(dtype).copy()


def dev_sums(vs, src, fmt, ss=None, base=0):
    """vs_bgr_channel_sums_batch on device memory: frames with rows of ss elements, the first frame `base` elements into its allocation; the
    sums between four guard values on either side -> (n, 3) uint64"""
    import torch
    src = np.ascontiguousarray(src)
    n, h, w, _ = src.shape
    ss = 3 * w if ss is None else ss
    host = np.full(base + n * h * ss, 77, src.dtype)                 # (padding that would change every sum if it were read)
    host[base:].reshape(n, h, ss)[:, :, :3 * w] = src.reshape(n, h, 3 * w)
    dsrc = _to_dev(host)
    dsum = _to_dev(np.full(3 * n + 8, SUMS_GUARD, np.uint64))
    torch.cuda.synchronize()
    vs.channel_sums_batch_device(dsrc.data_ptr() + base * src.dtype.itemsize, h * ss, n, w, h, ss, fmt, dsum.data_ptr() + 32)
    torch.cuda.synchronize()
    back = _back(dsum, np.uint64)
    assert (back[:4] == SUMS_GUARD).all() and (back[-4:] == SUMS_GUARD).all(), "the sums' neighbours were written"
    return back[4:-4].reshape(n, 3)


def dev_blend(vs, src, cf, maps, sums, feather, match, roi=None, border=None, maxv=None, ss=None, ds=None):
    """vs_bgr_image_warp_fill_blend_batch on device memory -> (n_out, rh, rw, 3); maps: (A, B, TX, TY) tuples; sums (n_src, 3) or None.  The
    destination is checked for writes outside the windows, the sums for any write at all"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    rx, ry, rw, rh = roi if roi is not None else (0, 0, w, h)
    ss = 3 * w if ss is None else ss
    ds = 3 * rw if ds is None else ds
    host = np.zeros((n_src, h, ss), dtype)
    host[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out, n_cand = idx.shape
    flat = [vs.Transform.of(*t) for row in maps for t in row]
    assert len(flat) == n_out * n_cand
    arr = (vs.Transform * len(flat))(*flat)
    dfs = (rh + 2 * G) * ds
    guard = 0x5A if esz == 1 else 0x5A5A
    dsrc, ddst = _to_dev(host), _to_dev(np.full(n_out * dfs + 8, guard, dtype))
    shost = None
    if sums is not None:
        shost = np.full(3 * n_src + 8, SUMS_GUARD, np.uint64)
        shost[4:-4] = np.asarray(sums, np.uint64).reshape(-1)
        dsum = _to_dev(shost)
    torch.cuda.synchronize()
    p = vs.FillBlendParams(int(feather), int(match))
    vs._check(vs.lib().vs_bgr_image_warp_fill_blend_batch(C.c_void_p(dsrc.data_ptr()), h * ss, n_src, w, h, ss, 3, 8 * esz, n_out, n_cand,
                                                          idx.ctypes.data_as(C.POINTER(C.c_int32)), arr,
                                                          C.c_void_p(dsum.data_ptr() + 32) if sums is not None else None, C.byref(p),
                                                          vs.BORDER_CONSTANT if border is None else border,
                                                          maxv if maxv is not None else (255 if esz == 1 else 65535), rx, ry, rw, rh,
                                                          C.c_void_p(ddst.data_ptr() + G * ds * esz), dfs, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    if sums is not None:
        assert np.array_equal(_back(dsum, np.uint64), shost), "the sums were written"
    back = _back(ddst, dtype)
    frames = back[:n_out * dfs].reshape(n_out, rh + 2 * G, ds)
    res = frames[:, G:G + rh, :3 * rw].reshape(n_out, rh, rw, 3).copy()
    frames[:, G:G + rh, :3 * rw] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination window were written"
    assert (frames[:, G + rh:] == guard).all(), "rows below a destination window were written"
    assert (frames[:, G:G + rh, 3 * rw:] == guard).all(), "the tail of a destination row was written"
    assert (back == guard).all()
    return res


def frames(rng, n, w, h, dtype, maxv):
    """smooth-ish content with noise on top, every frame at an exposure of its own (0.7 .. 1.3)"""
    base = rng.integers(0, maxv + 1, (n, h // 8 + 2, w // 8 + 2, 3))
    up = np.repeat(np.repeat(base, 8, 1), 8, 2)[:, :h, :w]
    f = np.clip(up + rng.integers(-3, 4, up.shape), 0, maxv).astype(np.float64)
    f *= rng.uniform(0.7, 1.3, (n, 1, 1, 1))
    return np.clip(np.rint(f), 0, maxv).astype(dtype)
