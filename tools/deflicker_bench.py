#!/usr/bin/env python3
"""Cost of the stabilizer's deflicker (vs_stabilizer_set_deflicker, vs_deflicker.hip): vs_stabilizer_process_batch on device-resident clips
(synth camera path, default jitter) at 1080p and 4K 8-bit and 4K 10-bit, deflicker 0 and deflicker N alternating in one process after a
warm-up call.

Clock: HIP events on the default stream around whole calls.  The call returns only after its own streams have drained, so the figure is the
call's duration as the host sees it: alignment, smoother, every launch and the final synchronisation included -- call-level, not kernel time.
Beside it: the bytes the passes move by their model -- per output frame and candidate two quarter-frame reads at step 4 (every fourth row, and of
those rows every cache line: the target's and the candidate's), and one read and one write of the output window for the gain pass (every
alignment of this clip succeeds: the lists are never cut short) -- and the fraction of the 8 TB/s peak that the added time per output frame
makes of them.  Kernel times come from a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/deflicker_bench.py --quick --cases 4k8 --deflickers 4
--deflickers 0 with VS_AMD_LIB pointing at another build of the library (and VS_AMD_LIB_PARTIAL=1 when that build lacks the new symbols) is
the A/B of the deflicker-off path: no setter is called for deflicker 0.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"1080p8": (1920, 1080, 8, 60), "4k8": (3840, 2160, 8, 40), "4k10": (3840, 2160, 10, 40)}
LAG = 10
PEAK = 8.0e12


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
    ap.add_argument("--crop", type=int, default=32)
    ap.add_argument("--deflickers", default="0,4")
    ap.add_argument("--step", type=int, default=0, help="0: the library's default")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    deflickers = [int(x) for x in a.deflickers.split(",")]
    crop = a.crop
    out = {"lib": os.path.basename(capi.LIB_PATH), "lag": LAG, "crop": crop, "reps": reps, "clock": "HIP events around whole calls (ms)", "cases": {}}
    for name in a.cases.split(","):
        w, h, bits, n = CASES[name]
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        torch.cuda.synchronize()
        res = {"w": w, "h": h, "bits": bits, "frames": n, "outputs": n - LAG}
        dout = torch.empty((n, h - 2 * crop, w - 2 * crop, 3), dtype=frames.dtype, device="cuda")
        handles = {}
        for d in deflickers:
            st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop)
            if d:
                st.set_deflicker(d, capi.deflicker_params(step=a.step) if a.step else None)
            handles[d] = st
        call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, fmt, dout.data_ptr()))  # noqa: E731
        for st in handles.values():
            call(st)                                                 # warm-up: slabs, rings, scratch, code objects
        times = {d: [] for d in deflickers}
        for _ in range(reps):
            for d in deflickers:                                       # alternating
                times[d].append(timed(lambda: call(handles[d])))
        for d in deflickers:
            v = sorted(times[d])
            res["deflicker%d_ms_per_call" % d] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
        fbytes = w * h * 3 * (1 if bits == 8 else 2)
        for d in deflickers:
            if not d:
                continue
            step = a.step or 4
            model = d * 2 * fbytes // min(step, 4) + 2 * (w - 2 * crop) * (h - 2 * crop) * 3 * (1 if bits == 8 else 2)
            row = {"model_bytes_per_output_frame": model}
            if 0 in deflickers:
                added = (res["deflicker%d_ms_per_call" % d]["median"] - res["deflicker0_ms_per_call"]["median"]) / (n - LAG)
                row["added_ms_per_output_frame"] = round(added, 5)
                row["fraction_of_peak"] = round(model / max(added * 1e-3, 1e-12) / PEAK, 4)
            res["deflicker%d" % d] = row
        out["cases"][name] = res
        del frames, dout, handles
        torch.cuda.empty_cache()
    line = json.dumps({"deflicker_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
