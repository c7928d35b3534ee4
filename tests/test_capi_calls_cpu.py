"""-m "not gpu": what the wrappers of video_stabilizer_amd/capi.py hand to the library, call for call, against tests/golden/capi_calls.json.

A stand-in takes the library's place (capi._lib): host-only entry points (parameter defaults, the error text, format queries, the ABI
version, the transform algebra) are delegated to the real library; every other call is recorded and answered with 0, a create call with a
dummy handle, and a destroy call is swallowed.  Nothing runs, so the cases are tiny and need no device.

A recorded call binds its arguments to the parameter names of include/vs_amd.h.  Numbers are stored by value, structs by their field values,
Transform and integer arrays by their values, None as null.  A pointer is stored as the array it points into -- shape, dtype, byte offset and
the sha256 of the array's bytes at call time -- or, where it points into none, as its integer value (the device forms get made-up addresses).
The arrays looked at are those capi._p converted and those the binding's own frames hold when the call is made (the fidelity roi origin and
the YCbCr plane addresses are formed by hand from arrays that never pass _p).  Beside the calls the wrapper's return value is stored.

The fixture is a recorded result of this project's own binding.  `python tests/test_capi_calls_cpu.py <a capi.py> [out.json]` writes it from
that binding module; it was written from the binding as it was before its marshalling was gathered into helpers, so the test shows that
the helpers hand over what the hand-written wrappers did."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _capi_header as H  # noqa: E402

ROOT = H.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_calls.json")
DUMMY_HANDLE = 0x5EED0000
_BYREF = type(C.byref(C.c_int()))

N_SRC, HH, WW, N_OUT, N_CAND = 3, 5, 7, 2, 3
SS, DS, GUARD, ROI = WW * 3 + 5, WW * 3 + 2, 0x5A, (1, 1, 4, 3)


# ---- the stand-in ------------------------------------------------------------------------------------------------------------------------
def _delegated(name):
    return (name.endswith("_params_default") or name.startswith("vs_format_") or name.startswith("vs_transform_")
            or name in ("vs_last_error", "vs_abi_version", "vs_sizeof_align_info"))


def _root(a):
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a


def _arrays_in(v, depth=2):
    if isinstance(v, np.ndarray):
        yield v
    elif depth and isinstance(v, (list, tuple)):
        for x in v:
            yield from _arrays_in(x, depth - 1)
    elif depth and hasattr(v, "__dict__") and not isinstance(v, type):
        for x in vars(v).values():
            yield from _arrays_in(x, depth - 1)


class StandIn:
    """in capi._lib's place: see the module's docstring.  hooks: {entry point: f(bound arguments)}, for the out-arguments a wrapper asserts on"""

    def __init__(self, real, capi):
        self._real, self._capi, self._protos = real, capi, H.prototypes()
        self.calls, self.converted, self.hooks, self.unset = [], [], {}, ()

    def __getattr__(self, name):
        if not name.startswith("vs_"):
            raise AttributeError(name)
        if _delegated(name):
            return getattr(self._real, name)
        return lambda *args: self._answer(name, args)

    def _known(self):
        """the arrays a pointer may point into: what _p converted, and what the binding's frames on the stack hold"""
        found = list(self.converted)
        f = sys._getframe(2)
        while f is not None:
            if f.f_globals.get("__name__") == self._capi.__name__:
                for v in f.f_locals.values():
                    found.extend(_arrays_in(v))
            f = f.f_back
        roots = {}
        for a in found:
            r = _root(a)
            roots[id(r)] = r
        return list(roots.values())

    def _pointer(self, addr, known, hashed):
        if not addr:
            return None
        for r in known:
            lo = r.ctypes.data
            if lo <= addr < lo + max(r.nbytes, 1):
                d = {"shape": list(r.shape), "dtype": str(r.dtype), "offset": addr - lo}
                if hashed:
                    d["sha256"] = hashlib.sha256(r.tobytes()).hexdigest()
                return d
        return int(addr)

    def _struct(self, s, known):
        out = {}
        for k, t in s._fields_:
            v = getattr(s, k)
            if t is C.c_void_p:
                out[k] = self._pointer(v, known, True)
            elif isinstance(v, C.Structure):
                out[k] = self._struct(v, known)
            elif isinstance(v, C.Array):
                out[k] = [self._struct(x, known) if isinstance(x, C.Structure) else x for x in v]
            else:
                out[k] = v
        return out

    def _arg(self, kind, v, known, hashed):
        if isinstance(v, _BYREF):
            v = v._obj
        if v is None:
            return None
        if isinstance(v, C.Structure):
            return self._struct(v, known)
        if isinstance(v, C.Array):
            return [self._struct(x, known) if isinstance(x, C.Structure) else x for x in v]
        if isinstance(v, C._Pointer):                                   # an int32 array handed over as POINTER(c_int32)
            arr = getattr(v, "_arr", None)
            assert isinstance(arr, np.ndarray), "a typed pointer that no numpy array stands behind"
            return {"dtype": str(arr.dtype), "values": arr.ravel().tolist()}
        if isinstance(v, C.c_void_p):
            return self._pointer(v.value, known, hashed)
        if isinstance(v, C._SimpleCData):                               # an out-argument: c_int, c_double
            return v.value
        if kind == "pointer":
            return self._pointer(int(v), known, hashed)
        return float(v) if kind in ("double", "float") else int(v)

    def _answer(self, name, args):
        if name.endswith("_destroy"):
            return None
        ret, params = self._protos[name]
        assert len(args) == len(params), (name, len(args), len(params))
        known = self._known()
        self.calls.append({"fn": name, "args": {p: self._arg(kind, v, known, p not in self.unset) for (p, kind), v in zip(params, args)}})
        if name in self.hooks:
            self.hooks[name](dict(zip((p for p, _ in params), args)))
        return DUMMY_HANDLE if name.endswith("_create") else 0


def _result(v, hashed):
    if isinstance(v, np.ndarray):
        d = {"shape": list(v.shape), "dtype": str(v.dtype)}
        if hashed:
            d["sha256"] = hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
        return d
    if isinstance(v, (list, tuple)):
        return [_result(x, hashed) for x in v]
    if isinstance(v, C.Array):
        return [_result(x, hashed) for x in v]
    if isinstance(v, C.Structure):
        return {k: _result(getattr(v, k), hashed) for k, _ in v._fields_}
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    assert v is None, type(v)
    return None


def record(capi, real, case):
    """one case under the stand-in -> {"calls": [...], "result": ...}, as json.loads would give it back"""
    standin = StandIn(real, capi)
    handles = []
    saved = capi._lib, capi._p

    def spy(a):
        if isinstance(a, np.ndarray):
            standin.converted.append(a)
        return saved[1](a)

    capi._lib, capi._p = standin, spy
    try:
        res = case(capi, standin, handles)
    finally:
        for h in handles:                    # a dummy handle must never reach the real library's destroy call
            h.h = None
        capi._lib, capi._p = saved
    hashed = not getattr(case, "unset_result", False)
    return json.loads(json.dumps({"calls": standin.calls, "result": _result(res, hashed)}))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
CASES = {}


def case(unset=(), unset_result=False):
    """unset: parameter names whose buffer the wrapper leaves uninitialised (np.empty): no hash of it; unset_result: nor of what it returns"""
    def deco(f):
        def run(vs, standin, handles):
            standin.unset = unset
            return f(vs, standin, handles)
        run.unset_result = unset_result
        CASES[f.__name__] = run
        return f
    return deco


def frames(dtype=np.uint8, n=N_SRC, h=HH, w=WW, c=3, seed=1):
    """seeded content, the same under every numpy"""
    hi = 256 if dtype == np.uint8 else 1024
    k = np.arange(n * h * w * max(c, 1), dtype=np.int64)
    shape = (n, h, w, c) if c else (n, h, w)
    return (((k * 2654435761 + seed * 97) >> 7) % hi).astype(dtype).reshape(shape)


def cands(vs, n_out=N_OUT, n_cand=N_CAND):
    cand_frame = [[(i + j) % N_SRC if (i, j) != (0, n_cand - 1) else -1 for j in range(n_cand)] for i in range(n_out)]
    cand_t = [[vs.Transform.of(0.001 * i, -0.002 * j, 0.5 * i + j, -0.25 * j) for j in range(n_cand)] for i in range(n_out)]
    return cand_frame, cand_t


def ts_of(vs, n):
    return [vs.Transform.of(0.001 * i, -0.002 * i, 0.5 + i, -0.25 * i) for i in range(n)]


PITCH = dict(src_stride=SS, dst_stride=DS, guard=GUARD)
DEV = dict(src=0x10000, dst=0x20000, aux=0x30000, aux2=0x40000)


def stabilizer(vs, handles, **kw):
    s = vs.Stabilizer(device=0, lag=3, crop_pixels=1, **kw)
    handles.append(s)
    return s


def aligner(vs, handles, **kw):
    a = vs.Aligner(device=0, **kw)
    handles.append(a)
    return a


# -- the warps
@case(unset=("dst",), unset_result=True)
def warp_batch(vs, R, hs):
    return vs.bgr_image_warp_batch(frames(), ts_of(vs, N_SRC), mode=vs.WARP_BILINEAR_CV, border=vs.BORDER_CONSTANT)


@case(unset=("dst",), unset_result=True)
def warp_batch_u16(vs, R, hs):
    return vs.bgr_image_warp_batch(frames(np.uint16), ts_of(vs, N_SRC), max_value=1023)


@case(unset=("dst",), unset_result=True)
def warp_roi_batch(vs, R, hs):
    return vs.bgr_image_warp_roi_batch(frames(), ts_of(vs, N_SRC), ROI)


@case()
def warp_batch_device_list(vs, R, hs):
    return vs.bgr_image_warp_batch_device(DEV["src"], N_SRC, WW, HH, 3, 8, ts_of(vs, N_SRC), DEV["dst"], stream=0x7000)


@case()
def warp_batch_device_array(vs, R, hs):
    arr = (vs.Transform * N_SRC)(*ts_of(vs, N_SRC))
    return vs.bgr_image_warp_batch_device(DEV["src"], N_SRC, WW, HH, 3, 16, arr, DEV["dst"], mode=vs.WARP_LANCZOS2_SEP, border=vs.BORDER_CONSTANT)


@case()
def fill_batch(vs, R, hs):
    return vs.bgr_image_warp_fill_batch(frames(), *cands(vs))


@case()
def fill_batch_pitched(vs, R, hs):
    return vs.bgr_image_warp_fill_batch(frames(), *cands(vs), roi=ROI, src_stride=SS, dst_stride=DS)


@case()
def fill_batch_empty(vs, R, hs):
    return vs.bgr_image_warp_fill_batch(frames(), [], [])


@case()
def channel_sums(vs, R, hs):
    return vs.channel_sums_batch(frames())


@case()
def channel_sums_pitched(vs, R, hs):
    return vs.channel_sums_batch(frames(np.uint16), fmt=vs.FMT_BGR12, src_stride=SS)


@case()
def channel_sums_device(vs, R, hs):
    return vs.channel_sums_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, DEV["aux"], stream=0x7000)


@case()
def fill_blend(vs, R, hs):
    return vs.bgr_image_warp_fill_blend_batch(frames(), *cands(vs))


@case()
def fill_blend_pitched(vs, R, hs):
    sums = np.arange(N_SRC * 3, dtype=np.uint64).reshape(N_SRC, 3) + 1000
    return vs.bgr_image_warp_fill_blend_batch(frames(), *cands(vs), sums=sums, feather=3, match=1, roi=ROI, **PITCH)


@case()
def fill_coverage(vs, R, hs):
    return vs.bgr_fill_coverage_batch(WW, HH, *cands(vs))


@case()
def fill_coverage_pitched(vs, R, hs):
    return vs.bgr_fill_coverage_batch(WW, HH, *cands(vs), roi=ROI, cov_stride=WW + 3, guard=GUARD)


@case()
def fill_coverage_device(vs, R, hs):
    return vs.bgr_fill_coverage_batch_device(WW, HH, *cands(vs), ROI, DEV["dst"], 3 * (WW + 3), WW + 3, stream=0x7000)


@case()
def inpaint(vs, R, hs):
    return vs.bgr_inpaint_batch(frames(), frames(c=0, seed=2) & 1)


@case()
def inpaint_pitched(vs, R, hs):
    return vs.bgr_inpaint_batch(frames(), frames(c=0, seed=2) & 1, stride=SS, mask_stride=WW + 3, guard=GUARD)


@case()
def inpaint_device(vs, R, hs):
    return vs.bgr_inpaint_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR10, DEV["aux"], HH * (WW + 3), WW + 3)


# -- deblur, denoise, rolling shutter
@case()
def sharpness(vs, R, hs):
    return vs.sharpness_batch(frames())


@case()
def sharpness_pitched(vs, R, hs):
    return vs.sharpness_batch(frames(), src_stride=SS)


@case()
def sharpness_device(vs, R, hs):
    return vs.sharpness_batch_device(DEV["src"], N_SRC, WW, HH, vs.FMT_BGR8, DEV["aux"])


SHARP = np.array([5, 7, 11], np.uint64)


@case()
def deblur(vs, R, hs):
    return vs.bgr_deblur_batch(frames(), SHARP, *cands(vs))


@case()
def deblur_pitched(vs, R, hs):
    return vs.bgr_deblur_batch(frames(), SHARP, *cands(vs), params=vs.deblur_params(sensitivity=0.5, max_ratio=3.0), **PITCH)


@case()
def deblur_pitched_u16(vs, R, hs):
    return vs.bgr_deblur_batch(frames(np.uint16), SHARP, *cands(vs), **PITCH)


@case()
def deblur_device(vs, R, hs):
    return vs.bgr_deblur_batch_device(DEV["src"], N_SRC, WW, HH, vs.FMT_BGR8, DEV["aux"], *cands(vs), DEV["dst"], params=vs.deblur_params(), stream=0x7000)


@case()
def denoise(vs, R, hs):
    return vs.denoise_batch(frames(), *cands(vs))


@case()
def denoise_pitched(vs, R, hs):
    return vs.denoise_batch(frames(), *cands(vs), params=vs.denoise_params(strength=16), fmt=vs.FMT_BGR8, **PITCH)


@case()
def denoise_device(vs, R, hs):
    return vs.denoise_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, *cands(vs), DEV["dst"], HH * DS, DS)


@case()
def rolling(vs, R, hs):
    return vs.rolling_batch(frames(), *cands(vs, n_cand=2))


@case()
def rolling_pitched(vs, R, hs):
    return vs.rolling_batch(frames(), *cands(vs, n_cand=2), params=vs.rolling_params(readout=0.8), **PITCH)


@case()
def rolling_device(vs, R, hs):
    return vs.rolling_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, *cands(vs, n_cand=2), DEV["dst"], HH * DS, DS,
                                   params=vs.rolling_params(readout=-0.5), stream=0x7000)


# -- lens, remap, resize
@case()
def lens_map(vs, R, hs):
    return vs.lens_map(vs.lens_params(WW, HH, k1=-0.2), WW, HH)


@case()
def lens_map_pitched(vs, R, hs):
    return vs.lens_map(vs.lens_params(WW, HH, k1=-0.2, zoom=1.05), WW, HH, map_stride=2 * WW + 3, guard=GUARD)


@case()
def lens_map_device(vs, R, hs):
    vs.lens_map_device(vs.lens_params(WW, HH), WW, HH, DEV["aux"])
    return vs.lens_map_device(vs.lens_params(WW, HH), WW, HH, DEV["aux"], map_stride=2 * WW + 3, stream=0x7000)


def positions(oh=4, ow=6):
    return (np.arange(oh * ow * 2, dtype=np.int32) * 5).reshape(oh, ow, 2)


@case()
def remap(vs, R, hs):
    return vs.remap_batch(frames(), positions())


@case()
def remap_pitched(vs, R, hs):
    return vs.remap_batch(frames(), positions(), border=vs.BORDER_CONSTANT, map_stride=2 * 6 + 3, **PITCH)


@case()
def remap_device(vs, R, hs):
    return vs.remap_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, DEV["aux"], 15, 6, 4, DEV["dst"], 4 * DS, DS, stream=0x7000)


@case()
def resize(vs, R, hs):
    return vs.resize_batch(frames(), 6, 4)


@case()
def resize_pitched(vs, R, hs):
    return vs.resize_batch(frames(), 6, 4, filter=vs.RESIZE_AREA, **PITCH)


@case()
def resize_device(vs, R, hs):
    return vs.resize_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, vs.RESIZE_AREA, DEV["dst"], 4 * DS, 6, 4, DS)


# -- YCbCr
def planes(dtype=np.uint8, mono=False):
    cw, ch = (WW + 1) >> 1, (HH + 1) >> 1
    y = frames(dtype, c=0, seed=3)
    return (y, None, None) if mono else (y, frames(dtype, h=ch, w=cw, c=0, seed=4), frames(dtype, h=ch, w=cw, c=0, seed=5))


@case()
def ycbcr_to_bgr_planar(vs, R, hs):
    return vs.ycbcr_to_bgr_batch(*planes())


@case()
def ycbcr_to_bgr_planar_pitched(vs, R, hs):
    return vs.ycbcr_to_bgr_batch(*planes(), y_stride=WW + 3, c_stride=5, dst_stride=DS, guard=GUARD)


@case()
def ycbcr_to_bgr_nv12(vs, R, hs):
    return vs.ycbcr_to_bgr_batch(*planes(), interleaved="nv12", y_stride=WW + 3, c_stride=11, dst_stride=DS, guard=GUARD)


@case()
def ycbcr_to_bgr_nv21(vs, R, hs):
    return vs.ycbcr_to_bgr_batch(*planes(np.uint16), interleaved="nv21")


@case()
def ycbcr_to_bgr_mono(vs, R, hs):
    return vs.ycbcr_to_bgr_batch(*planes(mono=True))


@case()
def ycbcr_to_bgr_device(vs, R, hs):
    p = vs.ycbcr_planes(DEV["src"], DEV["aux"], DEV["aux2"], WW + 3, 5, 1, (1, 1), HH * (WW + 3), 3 * 5)
    return vs.ycbcr_to_bgr_batch_device(p, N_SRC, WW, HH, vs.FMT_BGR8, DEV["dst"], HH * DS, DS, stream=0x7000)


@case()
def bgr_to_ycbcr_planar(vs, R, hs):
    return vs.bgr_to_ycbcr_batch(frames())


@case()
def bgr_to_ycbcr_planar_pitched(vs, R, hs):
    return vs.bgr_to_ycbcr_batch(frames(), src_stride=SS, y_stride=WW + 3, c_stride=5, guard=GUARD)


@case()
def bgr_to_ycbcr_nv12(vs, R, hs):
    return vs.bgr_to_ycbcr_batch(frames(), interleaved="nv12", src_stride=SS, y_stride=WW + 3, c_stride=11, guard=GUARD)


@case()
def bgr_to_ycbcr_nv21(vs, R, hs):
    return vs.bgr_to_ycbcr_batch(frames(np.uint16), sub=(1, 0), interleaved="nv21")


@case()
def bgr_to_ycbcr_mono(vs, R, hs):
    return vs.bgr_to_ycbcr_batch(frames(), mono=True, guard=GUARD)


@case()
def bgr_to_ycbcr_device(vs, R, hs):
    p = vs.ycbcr_planes(DEV["dst"], None, None, WW, 0, 1, (1, 1), HH * WW, 0)
    return vs.bgr_to_ycbcr_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, p)


# -- deflicker, scene cuts, fidelity, sharpening
@case()
def exposure_stats(vs, R, hs):
    return vs.exposure_stats_batch(frames(), *cands(vs))


@case()
def exposure_stats_pitched(vs, R, hs):
    return vs.exposure_stats_batch(frames(), *cands(vs), params=vs.deflicker_params(step=2), src_stride=SS)


@case()
def exposure_stats_device(vs, R, hs):
    return vs.exposure_stats_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, *cands(vs), DEV["aux"], stream=0x7000)


STATS = (np.arange(N_OUT * N_CAND * 8, dtype=np.uint64) + 3).reshape(N_OUT, N_CAND, 8)


@case()
def exposure_gains(vs, R, hs):
    return vs.exposure_gains_batch(STATS, WW, HH), vs.exposure_gains_batch(STATS, WW, HH, params=vs.deflicker_params(step=2))


@case()
def exposure_gains_device(vs, R, hs):
    return vs.exposure_gains_batch_device(DEV["aux"], N_OUT, N_CAND, WW, HH, DEV["aux2"], params=vs.deflicker_params(step=2), stream=0x7000)


@case()
def gain(vs, R, hs):
    return vs.bgr_gain_batch(frames(), np.arange(N_SRC * 4, dtype=np.uint32).reshape(N_SRC, 4) + 60000)


@case()
def gain_pitched(vs, R, hs):
    return vs.bgr_gain_batch(frames(), np.arange(N_SRC * 4, dtype=np.uint32).reshape(N_SRC, 4) + 60000, **PITCH)


@case()
def gain_device(vs, R, hs):
    return vs.bgr_gain_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, DEV["aux"], DEV["src"], HH * SS, SS, stream=0x7000)


PAIRS = [(0, 1), (2, 0)]


@case()
def scene_stats(vs, R, hs):
    return vs.scene_stats_batch(frames(), PAIRS, ts_of(vs, 2))


@case()
def scene_stats_pitched(vs, R, hs):
    return vs.scene_stats_batch(frames(), PAIRS, ts_of(vs, 2), params=vs.scene_params(step=2, threshold=40), src_stride=SS)


@case()
def scene_stats_no_pairs(vs, R, hs):
    return vs.scene_stats_batch(frames(), [], [])


@case()
def scene_stats_device(vs, R, hs):
    return vs.scene_stats_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, PAIRS, ts_of(vs, 2), DEV["aux"], params=vs.scene_params(step=1))


@case()
def scene_cuts(vs, R, hs):
    return vs.scene_cuts(np.array([[35, 100], [35, 9000]], np.uint64), WW, HH, vs.scene_params(step=1))


@case()
def fidelity_stats(vs, R, hs):
    return vs.fidelity_stats_batch(frames(), None, PAIRS)


@case()
def fidelity_stats_pitched(vs, R, hs):
    return vs.fidelity_stats_batch(frames(), frames(n=2, seed=6), [(0, 1), (2, 0)], a_stride=SS, b_stride=SS + 1, roi=ROI)


@case()
def fidelity_stats_one_batch_roi(vs, R, hs):
    a = frames(np.uint16)
    return vs.fidelity_stats_batch(a, a, PAIRS, a_stride=SS, roi=ROI)


@case()
def fidelity_stats_device(vs, R, hs):
    return vs.fidelity_stats_batch_device(DEV["src"], HH * SS, N_SRC, SS, DEV["dst"], HH * DS, 2, DS, WW, HH, vs.FMT_BGR8, PAIRS, DEV["aux"], stream=0x7000)


@case()
def fidelity_scores(vs, R, hs):
    return vs.fidelity_scores(np.arange(12, dtype=np.uint64).reshape(2, 6), WW, HH)


def window():
    return frames(n=2, h=ROI[3], w=ROI[2], seed=7)


@case()
def sharpen(vs, R, hs):
    return vs.sharpen_batch(window(), ts_of(vs, 2), WW, HH)


@case()
def sharpen_pitched(vs, R, hs):
    return vs.sharpen_batch(window(), ts_of(vs, 2), WW, HH, ROI[0], ROI[1], params=vs.sharpen_params(strength=24), src_stride=ROI[2] * 3 + 5,
                            dst_stride=ROI[2] * 3 + 2, guard=GUARD)


@case()
def sharpen_no_frames(vs, R, hs):
    return vs.sharpen_batch(window()[:0], [], WW, HH)


@case()
def sharpen_device(vs, R, hs):
    return vs.sharpen_batch_device(DEV["src"], HH * SS, 2, WW, HH, vs.FMT_BGR8, ts_of(vs, 2), ROI[0], ROI[1], ROI[2], ROI[3], SS, DEV["dst"], HH * DS, DS,
                                   params=vs.sharpen_params(), stream=0x7000)


# -- handles
@case()
def flow_jitter_device(vs, R, hs):
    f = vs.Flow(vs.flow_params(levels=2, winsize=9))
    hs.append(f)
    return f.jitter_device(DEV["src"], N_SRC, WW, HH, vs.FMT_BGR8), f.jitter_device(DEV["src"], N_SRC, WW, HH, vs.FMT_GRAY8, stride=WW + 1, frame_stride=99)


@case()
def flow_jitter(vs, R, hs):
    f = vs.Flow()
    hs.append(f)
    return f.jitter(frames()), f.jitter(frames(c=0))


@case()
def aligner_create(vs, R, hs):
    a = aligner(vs, hs, select_mode=vs.SELECT_STABLE, phase_correlate=1, pyramid_min_width=8, max_iters=7)
    a.set_select_mode(vs.SELECT_STL_HOST)
    a.set_batch_mode(vs.BATCH_SHARED)
    a.enable_timing()
    a.wait_stream(0x7000)
    a.reset()
    return a.select_mode()


@case()
def aligner_align_next(vs, R, hs):
    a = aligner(vs, hs)
    return a.align_next(frames()[0]), a.align_next(frames(c=0)[0]), a.align_next(frames(np.uint16)[0], fmt=vs.FMT_BGR12)


@case()
def aligner_align_batch(vs, R, hs):
    a = aligner(vs, hs)
    return a.align_batch(frames()), a.align_batch_device(DEV["src"], N_SRC, WW, HH, vs.FMT_BGR8), \
        a.align_batch_device(DEV["src"], N_SRC, WW, HH, vs.FMT_GRAY8, stride=WW + 1, frame_stride=99)


@case()
def aligner_align_clips(vs, R, hs):
    a = aligner(vs, hs)
    clips = frames(n=4)
    return a.align_clips(clips, 2), a.align_clips(4, 2, mem_ptr=DEV["src"], w=WW, h=HH, fmt=vs.FMT_BGR8), \
        a.align_clips(4, 2, mem_ptr=DEV["src"], w=WW, h=HH, fmt=vs.FMT_BGR8, raw=True), a.align_clips(clips, 2, raw=True)


@case()
def stabilizer_create_every_keyword(vs, R, hs):
    s = stabilizer(vs, hs, select_mode=vs.SELECT_STABLE, border_fill=2, deblur=2, deblur_params=vs.deblur_params(max_ratio=3.0), denoise=2,
                   denoise_params=vs.denoise_params(strength=16), fill_blend=(3, 1), deflicker=2, deflicker_params=vs.deflicker_params(step=2), inpaint=1,
                   rolling_shutter=0.5, lens=(vs.lens_params(WW, HH, k1=-0.1), WW, HH), scene_cut=True, sharpen=True, output_size=(6, 4, vs.RESIZE_AREA),
                   warp_mode=vs.WARP_BILINEAR_CV, warp_border=vs.BORDER_CONSTANT, pyramid_min_width=8, phase_correlate=1, enable_smoother=0)
    return s.params


@case()
def stabilizer_create_struct_keywords(vs, R, hs):
    s = stabilizer(vs, hs, scene_cut=vs.scene_params(step=2), sharpen=vs.sharpen_params(strength=8), deblur=1, denoise=1, deflicker=1)
    return s.delivered_size(WW, HH)


@case()
def stabilizer_setters(vs, R, hs):
    s = stabilizer(vs, hs)
    s.set_output_size(-1, -1)
    s.set_output_size(6, 4, vs.RESIZE_AREA)
    for params in (None, vs.sharpen_params(strength=8)):
        s.set_sharpen(params)
    for params in (None, vs.scene_params(threshold=40)):
        s.set_scene_cut(params)
    s.set_lens(None)
    s.set_lens(vs.lens_params(WW, HH, k1=-0.1, border=vs.BORDER_CONSTANT), WW, HH)
    for readout in (None, 0, 0.5):
        s.set_rolling_shutter(readout)
    s.set_inpaint()
    s.set_inpaint(0)
    for params in (None, vs.deflicker_params(step=2)):
        s.set_deflicker(2, params)
    for params in (None, vs.denoise_params(strength=16)):
        s.set_denoise(2, params)
    for params in (None, vs.deblur_params(sensitivity=0.5)):
        s.set_deblur(2, params)
    s.set_border_fill(2)
    s.set_fill_blend()
    s.set_fill_blend(3, 1)
    s.set_select_mode(vs.SELECT_STL_HOST)
    s.wait_stream(0x7000)
    s.reset()
    return None


@case()
def stabilizer_getters(vs, R, hs):
    s = stabilizer(vs, hs)
    return [s.get_output_size(), s.get_sharpen(), s.get_scene_cut(), s.scene_cuts(4), s.get_lens(), s.get_rolling_shutter(), s.get_inpaint(),
            s.get_deflicker(), s.get_denoise(), s.deblur(), s.border_fill(), s.fill_blend(), s.select_mode(), s.state()]


@case(unset=("out",))
def stabilizer_process(vs, R, hs):
    s = stabilizer(vs, hs)
    return s.process(frames()[0]), s.process(frames(np.uint16)[0], fmt=vs.FMT_BGR12)


@case()
def stabilizer_process_batch(vs, R, hs):
    s = stabilizer(vs, hs)
    out = np.full((N_SRC, HH - 2, WW - 2, 3), 9, np.uint8)
    return s.process_batch(frames()), s.process_batch(frames(), out=out), s.process_batch_device(DEV["src"], N_SRC, WW, HH, vs.FMT_BGR8, DEV["dst"])


@case()
def stabilizer_process_clips(vs, R, hs):
    s = stabilizer(vs, hs)
    return s.process_clips(frames(n=4), 2), s.process_clips_device(DEV["src"], 2, 2, WW, HH, vs.FMT_BGR8, DEV["dst"])


def _delivers(w, h):
    def hook(args):
        args["out_w"]._obj.value, args["out_h"]._obj.value = w, h
    return hook


@case()
def stabilizer_process_batch_ycbcr(vs, R, hs):
    s = stabilizer(vs, hs)
    R.hooks["vs_stabilizer_process_batch_ycbcr"] = _delivers(WW - 2, HH - 2)             # the wrapper asserts on what the library says it delivered
    return s.process_batch_ycbcr(*planes()), s.process_batch_ycbcr(*planes(), interleaved="nv12", out_interleaved=None, guard=GUARD), \
        s.process_batch_ycbcr(*planes(mono=True)), s.process_batch_ycbcr(*planes(np.uint16), out_sub=(0, 0), out_interleaved="nv21", out_mono=False)


@case()
def stabilizer_process_batch_ycbcr_device(vs, R, hs):
    s = stabilizer(vs, hs)
    pin = vs.ycbcr_planes(DEV["src"], DEV["aux"], DEV["aux"] + 1, WW, 8, 2, (1, 1), HH * WW, 3 * 8)
    pout = vs.ycbcr_planes(DEV["dst"], DEV["aux2"], DEV["aux2"] + 0x100, WW, 4, 1, (1, 1), HH * WW, 3 * 4)
    return s.process_batch_ycbcr_device(pin, N_SRC, WW, HH, vs.FMT_BGR8, pout)


# ---- the test ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrapper_hands_over_what_was_recorded(vs, recorded, name):
    real = vs.lib()
    got = record(vs, real, CASES[name])
    assert vs._lib is real                                      # the session's binding has the real library back
    want = recorded[name]
    assert [c["fn"] for c in got["calls"]] == [c["fn"] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w, g["fn"]
    assert got["result"] == want["result"]


# ---- the two defects: a short cand_t in a device form, a misspelt field ----------------------------------------------------------------
def _short(vs):
    cand_frame, cand_t = cands(vs)
    return cand_frame, [row[:-1] for row in cand_t]


DEVICE_CANDIDATE_FORMS = {
    "deblur": lambda vs, cf, ct: vs.bgr_deblur_batch_device(DEV["src"], N_SRC, WW, HH, vs.FMT_BGR8, DEV["aux"], cf, ct, DEV["dst"]),
    "denoise": lambda vs, cf, ct: vs.denoise_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, cf, ct, DEV["dst"], HH * DS, DS),
    "rolling": lambda vs, cf, ct: vs.rolling_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, [r[:2] for r in cf], [r[:1] for r in ct],
                                                          DEV["dst"], HH * DS, DS),
    "exposure_stats": lambda vs, cf, ct: vs.exposure_stats_batch_device(DEV["src"], HH * SS, N_SRC, WW, HH, SS, vs.FMT_BGR8, cf, ct, DEV["aux"]),
    "fill_coverage": lambda vs, cf, ct: vs.bgr_fill_coverage_batch_device(WW, HH, cf, ct, ROI, DEV["dst"], 3 * WW, WW),
}


@pytest.mark.parametrize("name", sorted(DEVICE_CANDIDATE_FORMS))
def test_device_form_refuses_a_short_candidate_list(vs, name):
    """cand_t shorter than cand_frame says: the library would read past the Transform array.  The wrapper raises, and no call was made"""
    made = []

    def run(capi, standin, handles):
        made.append(standin)
        with pytest.raises(AssertionError):
            DEVICE_CANDIDATE_FORMS[name](capi, *_short(capi))

    record(vs, vs.lib(), run)
    assert made[0].calls == []


PARAMS_CONSTRUCTORS = {"aligner_params": (), "stabilizer_params": (), "deblur_params": (), "denoise_params": (), "rolling_params": (), "lens_params": (8, 6),
                       "deflicker_params": (), "scene_params": (), "sharpen_params": (), "flow_params": ()}


@pytest.mark.parametrize("name", sorted(PARAMS_CONSTRUCTORS))
def test_params_constructor_refuses_a_name_that_is_no_field(vs, name):
    with pytest.raises(TypeError, match="has no field 'strenght'"):
        getattr(vs, name)(*PARAMS_CONSTRUCTORS[name], strenght=1)


def test_stabilizer_params_still_routes_aligner_fields(vs):
    p = vs.stabilizer_params(pyramid_min_width=8, lag=3)
    assert (p.aligner.pyramid_min_width, p.lag) == (8, 3)


# ---- writing the fixture -----------------------------------------------------------------------------------------------------------------
def _write(binding_path, out_path):
    os.environ.setdefault("VS_AMD_LIB", os.path.join(ROOT, "video_stabilizer_amd", "libvs_amd.so"))
    spec = importlib.util.spec_from_file_location("capi_recorded", binding_path)
    capi = importlib.util.module_from_spec(spec)
    sys.modules["capi_recorded"] = capi
    spec.loader.exec_module(capi)
    real = capi.lib()
    rows = ['%s: %s' % (json.dumps(name), json.dumps(record(capi, real, CASES[name]), sort_keys=True)) for name in sorted(CASES)]
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    print("%d cases -> %s (%d bytes)" % (len(rows), out_path, os.path.getsize(out_path)))


if __name__ == "__main__":
    _write(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else FIXTURE)
