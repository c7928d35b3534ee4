#!/usr/bin/env python3
"""Cost of the YCbCr conversions (vs_ycbcr_to_bgr_batch, vs_bgr_to_ycbcr_batch, vs_stabilizer_process_batch_ycbcr; vs_ycbcr.hip).

Kernel level: 32 device-resident 4K frames, 8 and 10 bit, I420 and NV12, both directions, beside a hipMemcpyAsync device-to-device of the
same model bytes (1.5 + 3 samples per pixel: what a conversion must read and write) in the same run -- the copy is the yardstick; reported
are the fraction of the 8 TB/s peak and the ratio to the copy.  Host fed: a 1080p x 240 and a 4K x 60 clip through
vs_stabilizer_process_batch from host BGR and through vs_stabilizer_process_batch_ycbcr from host I420, the same handle settings, into
buffers made beforehand -- frames/s of each and the ratio (does halving the bytes over the link pay?).  Parent commit: with --parent-lib
(the parent commit's libvs_amd.so, built from a second checkout and loaded next to this one) vs_stabilizer_process_batch on a
device-resident 1080p x 240 clip against it: the untouched path must sit inside the run's own min-max spread of the parent.

The arms alternate inside one process after a warm-up of each.  Clock: HIP events on the default stream around whole calls for the
device-resident arms, the host's wall clock around whole calls for the host-fed ones (they synchronise, and the CPU's share -- the copy into
the pinned mirror -- belongs to them); every figure is the median of the repetitions with min and max beside it.
Prints one JSON line and, with --out, writes it to a file (profiles/ycbcr_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
import numpy as np  # noqa: E402
from video_stabilizer_amd import capi, synth  # noqa: E402

N_KERNEL = 32
PEAK = 8.0e12
LAG, CROP = 10, 32


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def walled(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def alternate(arms, reps, clock):
    for fn in arms.values():                                         # warm-up: pools, held buffers, code objects
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            times[k].append(clock(fn))
    return {k: stats(v) for k, v in times.items()}


def device_planes(n, w, h, dtype, nv12):
    """dense 4:2:0 planes in device memory -> (tensors, YcbcrPlanes)"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    esz = 2 if dtype == torch.int16 else 1
    ty = torch.zeros((n, h, w), dtype=dtype, device="cuda")
    if nv12:
        tc = torch.zeros((n, ch, 2 * cw), dtype=dtype, device="cuda")
        return [ty, tc], capi.ycbcr_planes(ty.data_ptr(), tc.data_ptr(), tc.data_ptr() + esz, w, 2 * cw, 2, (1, 1), w * h, 2 * cw * ch)
    tu, tv = (torch.zeros((n, ch, cw), dtype=dtype, device="cuda") for _ in range(2))
    return [ty, tu, tv], capi.ycbcr_planes(ty.data_ptr(), tu.data_ptr(), tv.data_ptr(), w, cw, 1, (1, 1), w * h, cw * ch)


def kernel_level(reps, hip):
    out = {}
    for bits in (8, 10):
        w, h, n = 3840, 2160, N_KERNEL
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        back = torch.empty_like(frames)
        esz = 1 if bits == 8 else 2
        model = (w * h * 3 + w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)) * esz * n       # read + written, the whole call
        ca, cb = (torch.empty(model // 2, dtype=torch.uint8, device="cuda") for _ in range(2))
        arms = {"copy_d2d": lambda: hip.hipMemcpyAsync(C.c_void_p(cb.data_ptr()), C.c_void_p(ca.data_ptr()), C.c_size_t(model // 2), 3, None)}
        keep = []
        for name, nv12 in (("i420", False), ("nv12", True)):
            tens, desc = device_planes(n, w, h, frames.dtype, nv12)
            keep.append(tens)
            capi.bgr_to_ycbcr_batch_device(frames.data_ptr(), h * w * 3, n, w, h, w * 3, fmt, desc)      # real content in the planes
            arms["to_bgr_" + name] = (lambda d=desc: capi.ycbcr_to_bgr_batch_device(d, n, w, h, fmt, back.data_ptr(), h * w * 3, w * 3))
            arms["to_ycbcr_" + name] = (lambda d=desc: capi.bgr_to_ycbcr_batch_device(frames.data_ptr(), h * w * 3, n, w, h, w * 3, fmt, d))
        torch.cuda.synchronize()
        res = {"w": w, "h": h, "bits": bits, "frames": n, "model_bytes": model, "ms_per_call": alternate(arms, reps, timed)}
        copy_ms = res["ms_per_call"]["copy_d2d"]["median"]
        res["fraction_of_peak"] = {k: round(model / (v["median"] * 1e-3) / PEAK, 4) for k, v in res["ms_per_call"].items()}
        res["over_copy"] = {k: round(v["median"] / copy_ms, 4) for k, v in res["ms_per_call"].items() if k != "copy_d2d"}
        out["4k%d" % bits] = res
        del frames, back, ca, cb, keep
        torch.cuda.empty_cache()
    return out


def host_fed(reps):
    out = {}
    lib = capi.lib()
    for name, (w, h, n) in (("1080p_x240", (1920, 1080, 240)), ("4k_x60", (3840, 2160, 60))):
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=8, margin=64)
        tens, desc = device_planes(n, w, h, frames.dtype, False)
        capi.bgr_to_ycbcr_batch_device(frames.data_ptr(), h * w * 3, n, w, h, w * 3, capi.FMT_BGR8, desc)
        torch.cuda.synchronize()
        bgr = frames.cpu().numpy()
        y, u, v = (t.cpu().numpy() for t in tens)
        del frames, tens
        torch.cuda.empty_cache()
        ow, oh = w - 2 * CROP, h - 2 * CROP
        ocw, och = (ow + 1) // 2, (oh + 1) // 2
        out_bgr = np.zeros((n, oh, ow, 3), np.uint8)
        oy, ou, ov = np.zeros((n, oh, ow), np.uint8), np.zeros((n, och, ocw), np.uint8), np.zeros((n, och, ocw), np.uint8)
        pin = capi.ycbcr_planes(y.ctypes.data, u.ctypes.data, v.ctypes.data, w, (w + 1) // 2, 1, (1, 1), w * h, ((w + 1) // 2) * ((h + 1) // 2))
        pout = capi.ycbcr_planes(oy.ctypes.data, ou.ctypes.data, ov.ctypes.data, ow, ocw, 1, (1, 1), ow * oh, ocw * och)
        has = (C.c_int32 * n)()
        gw, gh = C.c_int(), C.c_int()
        sa, sb = (capi.Stabilizer(device=0, lag=LAG, crop_pixels=CROP) for _ in range(2))

        def from_bgr():
            sa.reset()
            capi._check(lib.vs_stabilizer_process_batch(sa.h, capi._p(bgr), h * w * 3, n, w, h, w * 3, capi.FMT_BGR8, capi.MEM_HOST, capi._p(out_bgr), oh * ow * 3, has,
                                                        C.byref(gw), C.byref(gh)))

        def from_i420():
            sb.reset()
            capi._check(lib.vs_stabilizer_process_batch_ycbcr(sb.h, C.byref(pin), n, w, h, capi.FMT_BGR8, capi.MEM_HOST, C.byref(pout), has, C.byref(gw), C.byref(gh)))
        ms = alternate({"host_bgr": from_bgr, "host_i420": from_i420}, reps, walled)
        res = {"w": w, "h": h, "frames": n, "lag": LAG, "crop": CROP, "ms_per_call": ms,
               "frames_per_s": {k: round(n / (v["median"] * 1e-3), 1) for k, v in ms.items()},
               "link_bytes_per_frame": {"host_bgr": 3 * (w * h + ow * oh), "host_i420": int(1.5 * (w * h + ow * oh))}}
        res["i420_over_bgr_frames_per_s"] = round(res["frames_per_s"]["host_i420"] / res["frames_per_s"]["host_bgr"], 4)
        out[name] = res
        del sa, sb
    return out


def against_parent(path, reps):
    """vs_stabilizer_process_batch on a device-resident 1080p x 240 clip: this library and the parent commit's, alternating"""
    w, h, n = 1920, 1080, 240
    frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=8, margin=64)
    dout = torch.empty((n, h - 2 * CROP, w - 2 * CROP, 3), dtype=frames.dtype, device="cuda")
    parent = C.CDLL(os.path.abspath(path))
    for name in ("vs_stabilizer_create", "vs_stabilizer_destroy", "vs_stabilizer_reset", "vs_stabilizer_process_batch"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = capi.SIGNATURES[name]
    params = capi.stabilizer_params(lag=LAG, crop_pixels=CROP)
    has = (C.c_int32 * n)()
    gw, gh = C.c_int(), C.c_int()

    def arm(lib):
        hnd = lib.vs_stabilizer_create(C.byref(params), 0)
        assert hnd

        def call():
            lib.vs_stabilizer_reset(hnd)
            r = lib.vs_stabilizer_process_batch(hnd, C.c_void_p(frames.data_ptr()), h * w * 3, n, w, h, w * 3, capi.FMT_BGR8, capi.MEM_DEVICE,
                                                C.c_void_p(dout.data_ptr()), (h - 2 * CROP) * (w - 2 * CROP) * 3, has, C.byref(gw), C.byref(gh))
            assert r > 0, r
        return call
    ms = alternate({"this": arm(capi.lib()), "parent": arm(parent)}, reps, timed)
    ratio = round(ms["this"]["median"] / ms["parent"]["median"], 4)
    return {"w": w, "h": h, "frames": n, "ms_per_call": ms, "this_over_parent": ratio,
            "inside_parent_spread": bool(ms["parent"]["min"] <= ms["this"]["median"] <= ms["parent"]["max"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--parent-lib", default="", help="libvs_amd.so built from the parent commit")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.restype, hip.hipMemcpyAsync.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = {"lib": os.path.basename(capi.LIB_PATH), "parent_lib": os.path.basename(a.parent_lib), "reps": a.reps, "host_reps": a.host_reps,
           "clock": "HIP events around whole calls (device-resident arms), wall clock around whole calls (host-fed arms); ms",
           "model": "1.5 + 3 samples per pixel, read plus written; the copy moves the same bytes (half read, half written)",
           "kernel": kernel_level(max(3, a.reps), hip)}
    if not a.skip_host:
        out["host_fed"] = host_fed(max(3, a.host_reps))
    if a.parent_lib:
        out["parent"] = against_parent(a.parent_lib, max(3, a.reps))
    line = json.dumps({"ycbcr_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
