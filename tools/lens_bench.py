#!/usr/bin/env python3
"""Cost of the lens-distortion correction (vs_bgr_remap_batch, vs_lens_map, vs_stabilizer_set_lens, vs_remap.hip).

Kernel-level: vs_bgr_remap_batch through a radial lens map on 32 device-resident 4K frames, 8-bit and 10-bit, at the slice lengths of --slices
(how many frames a workgroup takes a pixel through; the library's own length is an arm too), beside vs_bgr_image_warp_roi_batch in
VS_WARP_BILINEAR_CV on the same frames -- that call moves the same frame bytes (one frame in, one frame out) -- and, with --parent-lib, beside
the same warp call of a library built from the parent commit (loaded next to this one: what the pass's arrival cost the default path).  The
map itself is timed as an arm of its own.  The arms alternate inside one process after a warm-up of each.  Engine-level:
vs_stabilizer_process_batch on a device-resident 1080p x 240 clip with the pass on against the pass off, alternating.

Other slice lengths reach the library through its test hooks (VS_TEST_HOOKS=1, VS_TEST_REMAP_SLICE, read at every call).

Clock: HIP events on the default stream around whole calls; every figure is the median of --reps calls with min and max beside it.  Model
bytes: one frame read and one written per frame, plus the map (8 bytes per output pixel) once per slice group.  Kernel times and counters come
from profiler runs of their own, e.g.  rocprofv3 --pmc SQ_INSTS_VALU -d OUT -- python tools/lens_bench.py --quick --cases 4k8 --engine-frames 0
Prints one JSON line and, with --out, writes it to a file (profiles/lens_bench.json)."""
import argparse
import ctypes as C
import json
import os
import sys

os.environ["VS_TEST_HOOKS"] = "1"                   # (before the library loads: the gate is read once per process)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
import numpy as np  # noqa: E402
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"4k8": (3840, 2160, 8), "4k10": (3840, 2160, 10), "1080p8": (1920, 1080, 8)}
N_KERNEL = 32
PEAK = 8.0e12
LENS = dict(k1=-0.25, k2=0.05, p1=0.001, p2=-0.002, zoom=1.05)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def warp_call(lib, src_ptr, n, w, h, bits, ts, dst_ptr, maxv):
    """vs_bgr_image_warp_roi_batch, VS_WARP_BILINEAR_CV, the full frame as the window, device memory (enqueue only)"""
    r = lib.vs_bgr_image_warp_roi_batch(C.c_void_p(src_ptr), h * w * 3, n, w, h, w * 3, 3, bits, ts, capi.WARP_BILINEAR_CV, capi.BORDER_CONSTANT,
                                        maxv, 0, 0, w, h, C.c_void_p(dst_ptr), h * w * 3, w * 3, capi.MEM_DEVICE, None)
    if r != 0:
        raise RuntimeError("vs_bgr_image_warp_roi_batch: error %d" % r)


def remap_call(slice_len, src_ptr, n, w, h, fmt, map_ptr, dst_ptr):
    if slice_len:
        os.environ["VS_TEST_REMAP_SLICE"] = str(slice_len)
    else:
        os.environ.pop("VS_TEST_REMAP_SLICE", None)
    capi.remap_batch_device(src_ptr, h * w * 3, n, w, h, w * 3, fmt, map_ptr, 2 * w, w, h, dst_ptr, h * w * 3, w * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one timed call per arm (profiler runs)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="4k8,4k10")
    ap.add_argument("--slices", default="1,4,8,32")
    ap.add_argument("--parent-lib", default="", help="libvs_amd.so built from the parent commit")
    ap.add_argument("--engine-frames", type=int, default=240, help="0: skip the stabilizer run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    slices = [int(s) for s in a.slices.split(",") if s]
    lib = capi.lib()
    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        parent.vs_bgr_image_warp_roi_batch.restype, parent.vs_bgr_image_warp_roi_batch.argtypes = capi.SIGNATURES["vs_bgr_image_warp_roi_batch"]
    out = {"lib": os.path.basename(capi.LIB_PATH), "parent_lib": os.path.basename(a.parent_lib), "reps": reps, "lens": LENS, "library_slice": capi.REMAP_SLICE,
           "clock": "HIP events around whole calls (ms)", "kernel": {}, "engine": {}}
    rng = np.random.default_rng(3)
    for name in a.cases.split(","):
        w, h, bits = CASES[name]
        n = N_KERNEL
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        maxv = (1 << bits) - 1
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        dst = torch.empty_like(frames)
        dmap = torch.empty((h, w, 2), dtype=torch.int32, device="cuda")
        lens = capi.lens_params(w, h, **LENS)
        capi.lens_map_device(lens, w, h, dmap.data_ptr())
        torch.cuda.synchronize()
        motions = [capi.Transform.of(rng.uniform(-0.005, 0.005), rng.uniform(-0.01, 0.01), rng.uniform(-8, 8), rng.uniform(-8, 8)) for _ in range(n)]
        ts = (capi.Transform * n)(*motions)
        arms = {"remap": lambda: remap_call(0, frames.data_ptr(), n, w, h, fmt, dmap.data_ptr(), dst.data_ptr())}
        for s in slices:
            arms["remap_slice%d" % s] = (lambda s=s: remap_call(s, frames.data_ptr(), n, w, h, fmt, dmap.data_ptr(), dst.data_ptr()))
        arms["lens_map"] = lambda: capi.lens_map_device(lens, w, h, dmap.data_ptr())
        arms["warp_cv"] = lambda: warp_call(lib, frames.data_ptr(), n, w, h, 8 if bits == 8 else 16, ts, dst.data_ptr(), maxv)
        if parent is not None:
            arms["warp_cv_parent"] = lambda: warp_call(parent, frames.data_ptr(), n, w, h, 8 if bits == 8 else 16, ts, dst.data_ptr(), maxv)
        for fn in arms.values():                                     # warm-up: rings, code objects
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(reps):
            for k, fn in arms.items():                               # alternating
                times[k].append(timed(fn))
        os.environ.pop("VS_TEST_REMAP_SLICE", None)
        fbytes = w * h * 3 * (1 if bits == 8 else 2)
        res = {"w": w, "h": h, "bits": bits, "frames": n, "model_bytes_per_frame": 2 * fbytes, "map_bytes": 8 * w * h}
        for k in arms:
            res[k + "_ms_per_call"] = stats(times[k])
            if k != "lens_map":
                res[k + "_fraction_of_peak"] = round(2 * fbytes * n / (res[k + "_ms_per_call"]["median"] * 1e-3) / PEAK, 4)
        res["remap_over_warp_cv"] = round(res["remap_ms_per_call"]["median"] / res["warp_cv_ms_per_call"]["median"], 4)
        if parent is not None:
            res["warp_cv_over_parent"] = round(res["warp_cv_ms_per_call"]["median"] / res["warp_cv_parent_ms_per_call"]["median"], 4)
        out["kernel"][name] = res
        del frames, dst, dmap
        torch.cuda.empty_cache()
    if a.engine_frames > 0:
        w, h, n, lag, crop = 1920, 1080, a.engine_frames, 10, 32
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=8, margin=64)
        dout = torch.empty((n, h - 2 * crop, w - 2 * crop, 3), dtype=frames.dtype, device="cuda")
        torch.cuda.synchronize()
        handles = {"off": capi.Stabilizer(device=0, lag=lag, crop_pixels=crop),
                   "on": capi.Stabilizer(device=0, lag=lag, crop_pixels=crop, lens=(capi.lens_params(w, h, **LENS), w, h))}
        call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, capi.FMT_BGR8, dout.data_ptr()))  # noqa: E731
        for st in handles.values():
            call(st)                                                 # warm-up: slabs, rings, the map, code objects
        times = {k: [] for k in handles}
        for _ in range(max(1, reps // 3) if not a.quick else 1):
            for k, st in handles.items():                            # alternating
                times[k].append(timed(lambda: call(st)))
        res = {"w": w, "h": h, "frames": n, "outputs": n - lag, "lag": lag, "crop": crop}
        for k in handles:
            res[k + "_ms_per_call"] = stats(times[k])
        res["added_ms_per_frame"] = round((res["on_ms_per_call"]["median"] - res["off_ms_per_call"]["median"]) / n, 5)
        res["on_over_off"] = round(res["on_ms_per_call"]["median"] / res["off_ms_per_call"]["median"], 4)
        out["engine"]["1080p8"] = res
    line = json.dumps({"lens_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
