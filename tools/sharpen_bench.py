#!/usr/bin/env python3
"""Cost of the stabilizer's phase-compensated sharpening (vs_stabilizer_set_sharpen, vs_sharpen.hip): vs_stabilizer_process_batch on
device-resident clips (synth camera path, default jitter) at 1080p x 60 and 4K x 40, 8-bit -- sharpen off and on alternating in one process after
a warm-up call.

Clock: HIP events on the default stream around whole calls.  The call returns only after its own streams have drained, so the figure is the
call's duration as the host sees it: alignment, smoother, every launch and the final synchronisation included -- call-level, not kernel time.
The spread of the repeats (min .. max) is reported with every median: two figures agree when their ranges overlap.
Beside it, per case: the kernel-level call alone (vs_bgr_sharpen_batch on device memory over the clip's n output windows under a quarter-pixel
rotation: matrices, kernel) per frame, and a device-to-device copy of one window -- the pass's floor: it reads and writes each byte once -- both
by HIP events around `inner` repeats; their ratio is what the pass costs over its floor.
--modes off with VS_AMD_LIB pointing at another build of the library (and VS_AMD_LIB_PARTIAL=1 when that build lacks the new symbols) is the
A/B of the sharpen-off path: no setter is called for "off".  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"1080p8": (1920, 1080, 8, 60), "4k8": (3840, 2160, 8, 40)}
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
    ap.add_argument("--cases", default="1080p8,4k8")
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
        ow, oh = w - 2 * crop, h - 2 * crop
        res = {"w": w, "h": h, "bits": bits, "frames": n, "window": [ow, oh]}
        dout = torch.empty((n, oh, ow, 3), dtype=frames.dtype, device="cuda")
        handles = {}
        for m in modes:
            st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop)
            if m == "on":
                st.set_sharpen(capi.sharpen_params())
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
            if "off" in modes:
                added = res["on_ms_per_call"]["median"] - res["off_ms_per_call"]["median"]
                res["on_minus_off_ms_per_call"] = round(added, 3)
                res["on_minus_off_us_per_output_frame"] = round(1e3 * added / (n - LAG), 3)
            # the kernel-level call alone, and its floor
            inner = 1 if a.quick else 20
            esz = 1 if bits == 8 else 2
            ts = [capi.Transform.of(0.002, 0.003, 1.25, -0.75)] * n
            wins = dout                                              # the last call's output windows: real content, dense
            dst = torch.empty_like(wins)
            kern = lambda: [capi.sharpen_batch_device(wins.data_ptr(), oh * ow * 3, n, w, h, fmt, ts, crop, crop, ow, oh, ow * 3, dst.data_ptr(),  # noqa: E731
                                                      oh * ow * 3, ow * 3) for _ in range(inner)]
            copy = lambda: [dst[0].copy_(wins[0]) for _ in range(inner)]  # noqa: E731
            kern()
            copy()
            k = spread([1e3 * timed(kern) / inner / n for _ in range(reps)])
            c = spread([1e3 * timed(copy) / inner for _ in range(reps)])
            res["sharpen_call_us_per_frame"] = k
            res["d2d_copy_one_window_us"] = c
            res["sharpen_over_copy"] = round(k["median"] / c["median"], 3)
            res["window_bytes"] = ow * oh * 3 * esz
            res["sharpen_gb_per_s_read_plus_write"] = round(2e-3 * res["window_bytes"] / k["median"], 1)
        out["cases"][name] = res
        del frames, dout, handles
        torch.cuda.empty_cache()
    line = json.dumps({"sharpen_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
