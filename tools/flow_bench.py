#!/usr/bin/env python3
"""Time of the flow-based jitter score (vs_flow_jitter, vs_flow.hip) per frame pair at 1080p and 4K, device-resident BGR8 clips.

vs_flow_jitter synchronises its own stream before it returns, so the figure is a host clock around whole calls: every launch,
the per-pair statistic and its device-to-host copy included.  Per-kernel times come from a separate profiler run, e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/flow_bench.py --quick --sizes 1080p
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one timed call per size (profiler runs)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1080p,4k", help="comma list of 1080p, 4k")
    a = ap.parse_args()
    reps = 1 if a.quick else a.reps
    out = {}
    for name, (w, h, n) in (("1080p", (1920, 1080, 25)), ("4k", (3840, 2160, 13))):
        if name not in a.sizes.split(","):
            continue
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", margin=32)
        torch.cuda.synchronize()
        f = capi.Flow()
        f.jitter_device(frames.data_ptr(), n, w, h, capi.FMT_BGR8)            # warm-up: scratch, code objects
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            med, pm = f.jitter_device(frames.data_ptr(), n, w, h, capi.FMT_BGR8)
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        out[name] = {"frames": n, "pairs": n - 1, "ms_per_call_median": round(times[len(times) // 2], 3),
                     "ms_per_pair": round(times[len(times) // 2] / (n - 1), 4), "ms_per_pair_min": round(times[0] / (n - 1), 4),
                     "score_px": round(med, 4)}
        del f, frames
        torch.cuda.empty_cache()
    print(json.dumps({"flow_jitter": out}))


if __name__ == "__main__":
    main()
