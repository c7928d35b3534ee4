#!/usr/bin/env python3
"""Cost of the stabilizer's scene-cut detection (vs_stabilizer_set_scene_cut, vs_scene.hip): vs_stabilizer_process_batch on device-resident
clips (synth camera path, default jitter, one scene: no cut fires, every frame is measured) at 1080p and 4K 8-bit, and on a 1080p clip long
enough for the overlapped run path (time chunks, the next chunk's alignment in flight while the statistics are downloaded) -- detection off and
on alternating in one process after a warm-up call.

Clock: HIP events on the default stream around whole calls.  The call returns only after its own streams have drained, so the figure is the
call's duration as the host sees it: alignment, smoother, every launch and the final synchronisation included -- call-level, not kernel time.
The spread of the repeats (min .. max) is reported with every median: two figures agree when their ranges overlap.
Beside it, per case: the statistics call alone (vs_bgr_scene_stats_batch on device memory over the same n - 1 pairs: memset, entries, kernel)
and a device-to-device copy of one frame as the yardstick, both by HIP events around `inner` repeats.
--modes off with VS_AMD_LIB pointing at another build of the library (and VS_AMD_LIB_PARTIAL=1 when that build lacks the new symbols) is the
A/B of the detection-off path: no setter is called for "off".  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"1080p8": (1920, 1080, 8, 60), "4k8": (3840, 2160, 8, 40), "1080p8_long": (1920, 1080, 8, 144)}
LAG = 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one timed call per setting (profiler runs)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="1080p8,4k8,1080p8_long")
    ap.add_argument("--crop", type=int, default=32)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    modes = a.modes.split(",")
    crop = a.crop
    out = {"lib": os.path.basename(capi.LIB_PATH), "lag": LAG, "crop": crop, "reps": reps, "clock": "HIP events around whole calls (ms)", "cases": {}}
    for name in a.cases.split(","):
        w, h, bits, n = CASES[name]
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        torch.cuda.synchronize()
        res = {"w": w, "h": h, "bits": bits, "frames": n, "pairs": n - 1}
        dout = torch.empty((n, h - 2 * crop, w - 2 * crop, 3), dtype=frames.dtype, device="cuda")
        handles = {}
        for m in modes:
            st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop)
            if m == "on":
                st.set_scene_cut(capi.scene_params())
            handles[m] = st
        call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, fmt, dout.data_ptr()))  # noqa: E731
        for st in handles.values():
            call(st)                                                 # warm-up: slabs, rings, scratch, code objects
        times = {m: [] for m in modes}
        for _ in range(reps):
            for m in modes:                                          # alternating
                times[m].append(timed(lambda: call(handles[m])))
        for m in modes:
            res["%s_ms_per_call" % m] = spread(times[m])
        if "on" in modes:
            res["cuts_reported"] = handles["on"].scene_cuts()[0]
            if "off" in modes:
                added = res["on_ms_per_call"]["median"] - res["off_ms_per_call"]["median"]
                res["on_minus_off_ms_per_call"] = round(added, 3)
                res["on_minus_off_us_per_frame"] = round(1e3 * added / n, 3)
            # the statistics call alone, and the yardstick
            inner = 1 if a.quick else 20
            pairs = [(j - 1, j) for j in range(1, n)]
            ts = [capi.Transform.of(0.0, 0.0, 1.5, -0.5)] * (n - 1)
            dstats = torch.zeros((2 * (n - 1),), dtype=torch.int64, device="cuda")
            esz = 1 if bits == 8 else 2
            stats = lambda: [capi.scene_stats_batch_device(frames.data_ptr(), h * w * 3, n, w, h, w * 3, fmt, pairs, ts, dstats.data_ptr())  # noqa: E731
                             for _ in range(inner)]
            scratch = torch.empty_like(frames[0])
            copy = lambda: [scratch.copy_(frames[0]) for _ in range(inner)]  # noqa: E731
            stats()
            copy()
            res["stats_call_us_per_pair"] = spread([1e3 * timed(stats) / inner / (n - 1) for _ in range(reps)])
            res["d2d_copy_one_frame_us"] = spread([1e3 * timed(copy) / inner for _ in range(reps)])
            res["frame_bytes"] = w * h * 3 * esz
        out["cases"][name] = res
        del frames, dout, handles
        torch.cuda.empty_cache()
    line = json.dumps({"scene_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
