#!/usr/bin/env python3
"""Cost of the fidelity statistics (vs_bgr_fidelity_batch, vs_fidelity.hip): 32 consecutive frame pairs of a device-resident clip (synth camera
path, default jitter) per call, at 1080p and 4K, 8-bit and 10-bit; the statistics stay in device memory, the call only enqueues.

Clock: HIP events on the default stream around whole calls (`inner` calls between two events, after a warm-up call): memset, pair entries and the
kernel.  The median of `reps` repeats is reported with its min .. max: two figures agree when their ranges overlap.
Yardstick, in the same run: a device-to-device copy of one frame.  It moves the same bytes as a pair: a pair reads two frames, a copy reads one
and writes one.  No ratio is fixed in advance; `pair_over_copy` is what came out.  --inset C measures the frames minus C pixels a side (an odd
C: no row of the image starts on a dword, the sample-by-sample path).  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
from video_stabilizer_amd import capi, synth  # noqa: E402

CASES = {"1080p8": (1920, 1080, 8), "1080p10": (1920, 1080, 10), "4k8": (3840, 2160, 8), "4k10": (3840, 2160, 10)}
PAIRS = 32


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
    ap.add_argument("--quick", action="store_true", help="one timed call per case (profiler runs)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cases", default="1080p8,1080p10,4k8,4k10")
    ap.add_argument("--inset", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    inner = 1 if a.quick else 10
    out = {"lib": os.path.basename(capi.LIB_PATH), "pairs_per_call": PAIRS, "inset": a.inset, "reps": reps, "calls_per_timing": inner,
           "clock": "HIP events around whole calls", "cases": {}}
    for name in a.cases.split(","):
        w, h, bits = CASES[name]
        n = PAIRS + 1
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        esz = 1 if bits == 8 else 2
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        torch.cuda.synchronize()
        c = a.inset
        iw, ih = w - 2 * c, h - 2 * c
        org = frames.data_ptr() + (c * w * 3 + c * 3) * esz
        pairs = [(j, j + 1) for j in range(PAIRS)]
        dstats = torch.zeros((6 * PAIRS,), dtype=torch.int64, device="cuda")
        call = lambda: [capi.fidelity_stats_batch_device(org, h * w * 3, n, w * 3, org, h * w * 3, n, w * 3, iw, ih, fmt, pairs, dstats.data_ptr())  # noqa: E731
                        for _ in range(inner)]
        scratch = torch.empty_like(frames[0])
        copy = lambda: [scratch.copy_(frames[0]) for _ in range(inner)]  # noqa: E731
        call()
        copy()
        torch.cuda.synchronize()
        st = dstats.cpu().numpy().view("uint64").reshape(PAIRS, 6)
        sc = capi.fidelity_scores(st, iw, ih, fmt)
        per_pair = spread([1e3 * timed(call) / inner / PAIRS for _ in range(reps)])
        per_copy = spread([1e3 * timed(copy) / inner for _ in range(reps)])
        frame_bytes = w * h * 3 * esz
        res = {"w": w, "h": h, "bits": bits, "image": [iw, ih], "frame_bytes": frame_bytes, "pair_us": per_pair, "d2d_copy_one_frame_us": per_copy,
               "pair_over_copy": round(per_pair["median"] / per_copy["median"], 3),
               "pair_read_GBps": round(2 * iw * ih * 3 * esz / per_pair["median"] / 1e3, 1), "copy_GBps": round(2 * frame_bytes / per_copy["median"] / 1e3, 1),
               "itf_psnr_db": round(float(sum(min(v, 100.0) for v in sc[:, 3]) / PAIRS), 3), "itf_ssim": round(float(sc[:, 5].mean()), 4)}
        out["cases"][name] = res
        del frames, scratch
        torch.cuda.empty_cache()
    line = json.dumps({"fidelity_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
