#!/usr/bin/env python3
"""Cost of the resize pass (vs_bgr_resize_batch, vs_resize.hip) at the kernel level.

32 device-resident frames per shape, 8-bit and 10-bit: 4K -> 1080p under VS_RESIZE_AREA and under VS_RESIZE_LINEAR, and 3712 x 2032 ->
3840 x 2160 under VS_RESIZE_LINEAR (a crop of 64 zoomed back to the source size).  Arms per shape: the library's call as it ships, each kernel
form by name (the tiled form with H in LDS, the direct form; VS_TEST_HOOKS=1 and VS_TEST_RESIZE_FORM, read at every call), and a
device-to-device hipMemcpyAsync of source plus destination bytes.  The arms alternate inside one process after a warm-up of each.

Clock: HIP events on the default stream around whole calls; every figure is the median of --reps calls with min and max beside it.  Model
bytes of a resize: every source byte read once and every destination byte written once; the copy of B = source + destination bytes reads B
and writes B, twice the resize's model bytes, and its share of the peak is counted on 2 B.  touched: the fraction of the source's samples
that carry a non-zero weight (from vs_resize_taps) -- what a reader that skips the others could save.  With --check every arm's output is
compared with the first arm's.

Engine level: vs_stabilizer_process_batch on device-resident clips, 1080p x 60 and 4K x 40, lag 10, crop 32, with the output size off and
set to the source size, alternating.  Parent commit: with --parent-lib (the parent commit's libvs_amd.so, built from a second checkout and
loaded next to this one) the same call with the pass off on a 1080p x 240 clip against it: the untouched path must sit inside the run's own
min-max spread of the parent.  Prints one JSON line and, with --out, writes it to a file (profiles/resize_bench.json)."""
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

SHAPES = {"4k_to_1080p_area": (3840, 2160, 1920, 1080, capi.RESIZE_AREA), "4k_to_1080p_linear": (3840, 2160, 1920, 1080, capi.RESIZE_LINEAR),
          "crop64_to_4k_linear": (3712, 2032, 3840, 2160, capi.RESIZE_LINEAR)}
FORMS = {"tiled": 0, "direct": 1}
N_FRAMES = 32
PEAK = 8.0e12


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


def resize_call(form, src, dst, n, sw, sh, dw, dh, fmt, filt):
    if form is None:
        os.environ.pop("VS_TEST_RESIZE_FORM", None)
    else:
        os.environ["VS_TEST_RESIZE_FORM"] = str(form)
    capi.resize_batch_device(src.data_ptr(), sh * sw * 3, n, sw, sh, sw * 3, fmt, filt, dst.data_ptr(), dh * dw * 3, dw, dh, dw * 3)


def touched_fraction(s, d, filt):
    i0, n, wt = capi.resize_taps(s, d, filt)
    seen = np.zeros(s, bool)
    for k in range(int(n.max())):
        live = (n > k) & (wt[:, k] > 0)
        seen[(i0 + k)[live]] = True
    return float(seen.mean())


LAG, CROP = 10, 32


def alternate(arms, reps):
    for fn in arms.values():                                         # warm-up: pools, scratch, rings, code objects
        fn()
        fn()
    times = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            times[k].append(timed(fn))
    return {k: stats(v) for k, v in times.items()}


def engine_level(reps):
    out = {}
    for name, (w, h, n) in (("1080p_x60", (1920, 1080, 60)), ("4k_x40", (3840, 2160, 40))):
        frames, _ = synth.make_clip_torch(w, h, n, seed=3, device="cuda", bits=8, margin=64)
        dout = torch.empty((n, h, w, 3), dtype=frames.dtype, device="cuda")        # (large enough for either size)
        handles = {"off": capi.Stabilizer(device=0, lag=LAG, crop_pixels=CROP), "on": capi.Stabilizer(device=0, lag=LAG, crop_pixels=CROP, output_size=(-1, -1))}
        call = lambda st: (st.reset(), st.process_batch_device(frames.data_ptr(), n, w, h, capi.FMT_BGR8, dout.data_ptr()))  # noqa: E731
        ms = alternate({k: (lambda st=st: call(st)) for k, st in handles.items()}, reps)
        out[name] = {"w": w, "h": h, "frames": n, "outputs": n - LAG, "lag": LAG, "crop": CROP, "delivered": [w, h], "ms_per_call": ms,
                     "added_ms_per_output": round((ms["on"]["median"] - ms["off"]["median"]) / (n - LAG), 5),
                     "on_over_off": round(ms["on"]["median"] / ms["off"]["median"], 4)}
        del handles, frames, dout
        torch.cuda.empty_cache()
    return out


def against_parent(path, reps):
    """vs_stabilizer_process_batch on a device-resident 1080p x 240 clip, no output size set: this library and the parent commit's, alternating"""
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
    ms = alternate({"this": arm(capi.lib()), "parent": arm(parent)}, reps)
    return {"w": w, "h": h, "frames": n, "ms_per_call": ms, "this_over_parent": round(ms["this"]["median"] / ms["parent"]["median"], 4),
            "inside_parent_spread": bool(ms["parent"]["min"] <= ms["this"]["median"] <= ms["parent"]["max"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one timed call per arm (profiler runs)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--bits", default="8,10")
    ap.add_argument("--check", action="store_true", help="compare every arm's output with the first arm's")
    ap.add_argument("--engine", action="store_true", help="the stabilizer runs with the output size off and on")
    ap.add_argument("--parent-lib", default="", help="libvs_amd.so built from the parent commit")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    reps = 1 if a.quick else max(3, a.reps)
    hip = C.CDLL("libamdhip64.so")                                   # (the runtime torch has loaded)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    out = {"lib": os.path.basename(capi.LIB_PATH), "reps": reps, "frames": N_FRAMES, "clock": "HIP events around whole calls (ms)", "peak_bytes_per_s": PEAK,
           "shapes": {}}
    for name in [s for s in a.shapes.split(",") if s]:
        sw, sh, dw, dh, filt = SHAPES[name]
        for bits in [int(b) for b in a.bits.split(",")]:
            n = N_FRAMES
            fmt = capi.FMT_BGR8 if bits == 8 else capi.FMT_BGR10
            esz = 1 if bits == 8 else 2
            src, _ = synth.make_clip_torch(sw, sh, n, seed=3, device="cuda", bits=bits, margin=64)
            dst = torch.empty((n, dh, dw, 3), dtype=src.dtype, device="cuda")
            sbytes, dbytes = n * sw * sh * 3 * esz, n * dw * dh * 3 * esz
            ca, cb = torch.empty(sbytes + dbytes, dtype=torch.uint8, device="cuda"), torch.empty(sbytes + dbytes, dtype=torch.uint8, device="cuda")
            arms = {"resize": lambda: resize_call(None, src, dst, n, sw, sh, dw, dh, fmt, filt)}
            for fname, form in FORMS.items():
                arms["resize_" + fname] = (lambda form=form: resize_call(form, src, dst, n, sw, sh, dw, dh, fmt, filt))
            arms["copy"] = lambda: hip.hipMemcpyAsync(cb.data_ptr(), ca.data_ptr(), sbytes + dbytes, 3, None)
            first = None
            for k, fn in arms.items():                                   # warm-up: rings, code objects
                fn()
                fn()
                torch.cuda.synchronize()
                if a.check and k != "copy":
                    got = dst.clone()
                    first = got if first is None else first
                    assert torch.equal(got, first), "arm %s differs from the first arm" % k
                    dst.zero_()
            times = {k: [] for k in arms}
            for _ in range(reps):
                for k, fn in arms.items():                               # alternating
                    times[k].append(timed(fn))
            os.environ.pop("VS_TEST_RESIZE_FORM", None)
            res = {"sw": sw, "sh": sh, "dw": dw, "dh": dh, "filter": "area" if filt == capi.RESIZE_AREA else "linear", "bits": bits,
                   "model_bytes": sbytes + dbytes, "copy_moves_bytes": 2 * (sbytes + dbytes),
                   "touched": round(touched_fraction(sw, dw, filt) * touched_fraction(sh, dh, filt), 4)}
            for k in arms:
                res[k + "_ms_per_call"] = stats(times[k])
                moved = (2 if k == "copy" else 1) * (sbytes + dbytes)
                res[k + "_fraction_of_peak"] = round(moved / (res[k + "_ms_per_call"]["median"] * 1e-3) / PEAK, 4)
                if k != "copy":
                    res[k + "_over_copy"] = round(res[k + "_ms_per_call"]["median"] / stats(times["copy"])["median"], 4)
            out["shapes"]["%s_%d" % (name, bits)] = res
            del src, dst, ca, cb
            torch.cuda.empty_cache()
    if a.engine:
        out["engine"] = engine_level(max(3, reps // 2))
    if a.parent_lib:
        out["parent_lib"] = os.path.basename(a.parent_lib)
        out["parent"] = against_parent(a.parent_lib, reps)
    line = json.dumps({"resize_bench": out})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
