#!/usr/bin/env python3
"""Cost of the stabilizer's border fill (vs_stabilizer_set_border_fill, vs_fill.hip): vs_stabilizer_process_batch on device-resident clips
(synth camera path, default jitter) at 1080p and 4K 8-bit and 4K 10-bit, crop_pixels 32 and 0, fill 0 and fill N alternating in one process
after a warm-up call.

Clock: HIP events on the default stream around whole calls.  The call returns only after its own streams have drained, so the figure is the
call's duration as the host sees it: alignment, smoother, every launch and the final synchronisation included -- call-level, not kernel time.
Beside it: (a) the fixed-point bilinear warp alone on the same clip (vs_bgr_image_warp_batch, same clock) per frame, and (b) the share of the
fill kernel's 64 x 16 output strips that hold a pixel the frame's own correction does not cover, counted on the host from the corrections of
a frame-by-frame run.  Kernel times come from a profiler run of its own, e.g.
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/fill_bench.py --quick --cases 4k8 --fills 4
--fills 0 with VS_AMD_LIB pointing at another build of the library is the A/B of the fill-off path (a library without the feature: no setter
is called for fill 0).  Prints one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def uncovered_strips(t, w, h, crop):
    """(strips with an uncovered pixel, strips) of the output window for the forward transform t: the table rule on whole rows / columns"""
    M = capi.cv_inverse_matrix(t, w, h)
    xs = np.arange(crop, w - crop, dtype=np.float64)
    ys = np.arange(crop, h - crop, dtype=np.float64)
    ad, bd = np.rint(M[0] * xs * 1024).astype(np.int64), np.rint(M[3] * xs * 1024).astype(np.int64)
    X0, Y0 = np.rint((M[1] * ys + M[2]) * 1024).astype(np.int64) + 16, np.rint((M[4] * ys + M[5]) * 1024).astype(np.int64) + 16

    def lo_hi(v, step):
        pad = (-len(v)) % step
        v = np.concatenate([v, np.repeat(v[-1:], pad)]).reshape(-1, step)
        return v.min(1), v.max(1)
    (adl, adh), (bdl, bdh), (Xl, Xh), (Yl, Yh) = lo_hi(ad, 64), lo_hi(bd, 64), lo_hi(X0, 16), lo_hi(Y0, 16)
    ok = ((((Xl[:, None] + adl[None, :]) >> 10) >= 0) & (((Xh[:, None] + adh[None, :]) >> 10) + 1 <= w - 1) &
          (((Yl[:, None] + bdl[None, :]) >> 10) >= 0) & (((Yh[:, None] + bdh[None, :]) >> 10) + 1 <= h - 1))
    return int((~ok).sum()), int(ok.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one timed call per setting (profiler runs)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="1080p8,4k8,4k10")
    ap.add_argument("--crops", default="32,0")
    ap.add_argument("--fills", default="0,4")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    fills = [int(x) for x in a.fills.split(",")]
    out = {"lib": os.path.basename(capi.LIB_PATH), "lag": LAG, "reps": reps, "clock": "HIP events around whole calls (ms)", "cases": {}}
    for name in a.cases.split(","):
        w, h, bits, n = CASES[name]
        fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=bits, margin=64)
        torch.cuda.synchronize()
        res = {"w": w, "h": h, "bits": bits, "frames": n, "outputs": n - LAG}
        # (a) the warp alone, all n frames of the clip in one call
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
            handles = {}
            for f in fills:
                st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop)
                if f:
                    st.set_border_fill(f)
                handles[f] = st
            call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, fmt, dout.data_ptr()))  # noqa: E731
            for st in handles.values():
                call(st)                                             # warm-up: slabs, rings, code objects
            times = {f: [] for f in fills}
            for _ in range(reps):
                for f in fills:                                      # alternating
                    times[f].append(timed(lambda: call(handles[f])))
            row = {}
            for f in fills:
                v = sorted(times[f])
                row["fill%d_ms_per_call" % f] = {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}
            if 0 in fills and len(fills) > 1:
                for f in fills:
                    if f:
                        row["fill%d_added_ms_per_output_frame" % f] = round(
                            (row["fill%d_ms_per_call" % f]["median"] - row["fill0_ms_per_call"]["median"]) / (n - LAG), 5)
            # (b) strips with an uncovered pixel, from the corrections of a frame-by-frame run (the fill does not change them)
            st = capi.Stabilizer(device=0, lag=LAG, crop_pixels=crop)
            bad = tot = 0
            for i in range(n):
                r, has = st.process_batch_device(frames[i].data_ptr(), 1, w, h, fmt, dout.data_ptr())
                if has[0]:
                    b, t = uncovered_strips(capi.t_inverse(st.state()[1]), w, h, crop)
                    bad, tot = bad + b, tot + t
            row["uncovered_strip_share"] = round(bad / max(tot, 1), 5)
            res["crop%d" % crop] = row
            del dout, handles, st
        out["cases"][name] = res
        del frames
        torch.cuda.empty_cache()
    print(json.dumps({"fill_bench": out}))


if __name__ == "__main__":
    main()
