#!/usr/bin/env python3
"""Cost of the stabilizer's inpaint (vs_stabilizer_set_inpaint, vs_inpaint.hip): vs_stabilizer_process_batch on device-resident clips (synth
camera path, default jitter) at 1080p and 4K 8-bit and 4K 10-bit, crop_pixels 32 and 0, border fill 0 and 4, inpaint off and on alternating
in one process after a warm-up call.

Clock: HIP events on the default stream around whole calls.  The call returns only after its own streams have drained, so the figure is the
call's duration as the host sees it: alignment, smoother, every launch and the final synchronisation included -- call-level, not kernel time.
Beside it: the fixed-point bilinear warp alone on the same clip (vs_bgr_image_warp_batch, same clock) per frame -- column (a) of the border
fill's table (tools/fill_bench.py).  Kernel times come from a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/inpaint_bench.py --quick --cases 4k8 --fills 4 --crops 0
--inpaints 0 with VS_AMD_LIB pointing at another build of the library is the A/B of the inpaint-off path (a library without the feature:
no setter is called for inpaint 0).  Prints one JSON line; --out FILE writes it there as well."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"1080p8": (1920, 1080, 8, 60), "4k8": (3840, 2160, 8, 40), "4k10": (3840, 2160, 10, 40)}
LAG = 10


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one timed call per setting (profiler runs)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="1080p8,4k8,4k10")
    ap.add_argument("--crops", default="32,0")
    ap.add_argument("--fills", default="0,4")
    ap.add_argument("--inpaints", default="0,1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    fills = [int(x) for x in a.fills.split(",")]
    inpaints = [int(x) for x in a.inpaints.split(",")]
    out = {"lib": os.path.basename(capi.LIB_PATH), "lag": LAG, "reps": reps, "clock": "HIP events around whole calls (ms)", "cases": {}}
    for name in a.cases.split(","):
        w, h, bits, n = CASES[name]
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        torch.cuda.synchronize()
        res = {"w": w, "h": h, "bits": bits, "frames": n, "outputs": n - LAG}
        ts = [capi.Transform.of(0.001, -0.002, 3.25, -2.5)] * n
        wout = torch.empty_like(frames)
        warp = lambda: capi.bgr_image_warp_batch_device(frames.data_ptr(), n, w, h, 3, 8 if bits == 8 else 16, ts, wout.data_ptr(),  # noqa: E731
                                                        mode=capi.WARP_BILINEAR_CV, border=capi.BORDER_CONSTANT, max_value=(1 << bits) - 1)
        warp()
        wt = sorted(timed(warp) for _ in range(reps))
        res["cv_warp_ms_per_frame_median"] = round(wt[len(wt) // 2] / n, 5)
        del wout
        for crop in [int(x) for x in a.crops.split(",")]:
            dout = torch.empty((n, h - 2 * crop, w - 2 * crop, 3), dtype=frames.dtype, device="cuda")
            for f in fills:
                handles = {}
                for ip in inpaints:
                    st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop)
                    if f:
                        st.set_border_fill(f)
                    if ip:
                        st.set_inpaint(1)
                    handles[ip] = st
                call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, fmt, dout.data_ptr()))  # noqa: E731
                for st in handles.values():
                    call(st)                                         # warm-up: slabs, rings, code objects, the scratch block
                times = {ip: [] for ip in inpaints}
                for _ in range(reps):
                    for ip in inpaints:                              # alternating
                        times[ip].append(timed(lambda: call(handles[ip])))
                row = {}
                for ip in inpaints:
                    v = sorted(times[ip])
                    row["inpaint%d_ms_per_call" % ip] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
                if 0 in inpaints and 1 in inpaints:
                    row["inpaint_added_ms_per_output_frame"] = round(
                        (row["inpaint1_ms_per_call"]["median"] - row["inpaint0_ms_per_call"]["median"]) / (n - LAG), 5)
                res["crop%d_fill%d" % (crop, f)] = row
                del handles
            del dout
        out["cases"][name] = res
        del frames
        torch.cuda.empty_cache()
    line = json.dumps({"inpaint_bench": out})
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps({"inpaint_bench": out}, indent=1) + "\n")


if __name__ == "__main__":
    main()
