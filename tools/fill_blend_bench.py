#!/usr/bin/env python3
"""Cost of the border fill's seam blend (vs_stabilizer_set_fill_blend, vs_fill.hip): vs_stabilizer_process_batch on device-resident clips (synth
camera path, default jitter) at 1080p and 4K 8-bit and 4K 10-bit, crop_pixels 32 and 0, with fill 4 and with fill 4 plus blend {feather 4, match 1},
alternating in one process after a warm-up call (tools/fill_bench.py's protocol and clock).

Clock: HIP events on the default stream around whole calls.  The call returns only after its own streams have drained, so the figure is the
call's duration as the host sees it: alignment, smoother, every launch (with the blend: the channel sums at ingest, the gain kernel, the blend
kernel in place of the fill kernel) and the final synchronisation included -- call-level, not kernel time.  "added" = (blend - fill) / output
frames.  Kernel times come from a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/fill_blend_bench.py --quick --cases 4k8 --crops 0
--no-blend with VS_AMD_LIB pointing at another build of the library is the A/B of the blend-off path (a library without the feature: no blend
setter is called).  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"1080p8": (1920, 1080, 8, 60), "4k8": (3840, 2160, 8, 40), "4k10": (3840, 2160, 10, 40)}
LAG, FILL = 10, 4


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
    ap.add_argument("--feather", type=int, default=4)
    ap.add_argument("--match", type=int, default=1)
    ap.add_argument("--no-blend", action="store_true", help="time fill 4 alone and call no blend setter (A/B against a library without it)")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    settings = ["fill"] if a.no_blend else ["fill", "blend"]
    out = {"lib": os.path.basename(capi.LIB_PATH), "lag": LAG, "fill": FILL, "blend": [a.feather, a.match], "reps": reps,
           "clock": "HIP events around whole calls (ms)", "cases": {}}
    for name in a.cases.split(","):
        w, h, bits, n = CASES[name]
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        torch.cuda.synchronize()
        res = {"w": w, "h": h, "bits": bits, "frames": n, "outputs": n - LAG}
        for crop in [int(x) for x in a.crops.split(",")]:
            dout = torch.empty((n, h - 2 * crop, w - 2 * crop, 3), dtype=frames.dtype, device="cuda")
            handles = {}
            for s in settings:
                st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop, border_fill=FILL)
                if s == "blend":
                    st.set_fill_blend(a.feather, a.match)
                handles[s] = st
            call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, fmt, dout.data_ptr()))  # noqa: E731
            for st in handles.values():
                call(st)                                             # warm-up: slabs, rings, code objects
            times = {s: [] for s in settings}
            for _ in range(reps):
                for s in settings:                                   # alternating
                    times[s].append(timed(lambda: call(handles[s])))
            row = {}
            for s in settings:
                v = sorted(times[s])
                row["%s_ms_per_call" % s] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
            if "blend" in settings:
                row["blend_added_ms_per_output_frame"] = round((row["blend_ms_per_call"]["median"] - row["fill_ms_per_call"]["median"]) / (n - LAG), 5)
            res["crop%d" % crop] = row
            del dout, handles
        out["cases"][name] = res
        del frames
        torch.cuda.empty_cache()
    print(json.dumps({"fill_blend_bench": out}))


if __name__ == "__main__":
    main()
