"""The float-tile Lanczos2 warps (VS_WARP_LANCZOS2_SEP, VS_WARP_LANCZOS2_FAST) read their tiles' windows and their rows' position terms from
per-launch tables (video_stabilizer_amd/csrc/vs_warp.hip: vs_k_warp_c3_tables).  Every sample must still be the oracle twin's, bit for bit:
np.array_equal against WARP_LANCZOS2_SEPARABLE / WARP_LANCZOS2_CONTRACTED, nothing looser.

Covered: the single-frame entry and the device batch entry (1 and 5 frames per call, every frame with its own transform), 8-bit and 10-bit
frames, clamp and constant border, windows of one tile (64 x 16), of four tiles with 1-pixel remnants (65 x 17), of several tiles with a last row
block of one row (130 x 37), narrower than a column group (3 x 5), and a window with odd offsets cut out of a larger frame; transforms that take
each window shape of the launcher (seven-wave, six-wave, standard), that leave the window (per-pixel path), that put whole tiles outside the
frame, whose fractions are exactly 0, and batches that mix shapes, so that the launcher must fall back to the standard one for all frames."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(64, 16), (65, 17), (130, 37), (3, 5)]
ROI_CASE = ((130, 37), (3, 5, 61, 14))


def _rot(deg, scale=1.0, tx=0.0, ty=0.0):
    a = math.radians(deg)
    return (scale * math.cos(a) - 1.0, scale * math.sin(a), tx, ty)


# name -> (A, B, TX, TY)
TRANSFORMS = {
    "identity": (0.0, 0.0, 0.0, 0.0),
    "integer_shift": (0.0, 0.0, 3.0, -2.0),                 # fractions exactly 0: the |x| >= 2 selects fire
    "small": (0.002, -0.001, 1.25, -0.75),                  # the seven-wave window (separable) / six-wave (contracted)
    "small_b": (-0.0015, 0.002, -2.6, 0.4),
    "small_c": (0.001, 0.0025, 0.55, 3.3),
    "zoom_1.035": _rot(0.1, 1.035, -0.3, 0.7),              # rows fit 20, columns need 80: the six-wave window
    "rot_1.2": _rot(1.2, 1.0, 0.4, -0.6),                   # just beyond the compact windows
    "rot_5": _rot(5.0, 1.0, -1.3, 2.2),                     # the standard window
    "rot_45_x1.4": _rot(45.0, 1.4, 0.25, 0.5),              # no window fits: the per-pixel path
    "tiles_outside": (0.0, 0.0, 70.5, -20.25),              # whole tiles sample beyond the frame
    "tiles_outside_b": (0.001, 0.0, -90.25, 30.5),
}
# five frames per call, each frame its own transform
BATCHES = {
    "seven_wave": ["identity", "integer_shift", "small", "small_b", "small_c"],
    "six_wave": ["zoom_1.035", "small", "identity", "zoom_1.035", "small_b"],
    "mixed_standard": ["small", "rot_5", "rot_1.2", "rot_45_x1.4", "tiles_outside"],     # a seven-wave frame beside a 5 degree one
    "outside": ["tiles_outside_b", "tiles_outside", "integer_shift", "small_c", "tiles_outside_b"],
}

_cache = {}


def _frames(w, h, bits):
    key = ("src", w, h, bits)
    if key not in _cache:
        rng = np.random.default_rng(1000 * w + 10 * h + bits)
        hi = 256 if bits == 8 else 1024
        _cache[key] = rng.integers(0, hi, (5, h, w, 3)).astype(np.uint8 if bits == 8 else np.uint16)
    return _cache[key]


def _want(O, w, h, bits, frame, name, omode, border):
    """the oracle twin's whole warped frame: computed once, shared, never written to"""
    key = (w, h, bits, frame, name, omode, border)
    if key not in _cache:
        out = O.bgr_image_warp(_frames(w, h, bits)[frame], O.Transform.of(*TRANSFORMS[name]), omode, border=border, max_value=255 if bits == 8 else 1023)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _modes(vs, O):
    return [(vs.WARP_LANCZOS2_SEP, O.WARP_LANCZOS2_SEPARABLE, "separable"), (vs.WARP_LANCZOS2_FAST, O.WARP_LANCZOS2_CONTRACTED, "contracted")]


def _borders(vs, O):
    return [(vs.BORDER_CLAMP, O.BORDER_CLAMP, "clamp"), (vs.BORDER_CONSTANT, O.BORDER_CONSTANT, "constant")]


def _device_batch(vs, torch, src, names, mode, border, maxv):
    n, h, w, _ = src.shape
    bits = 8 if src.dtype == np.uint8 else 16
    dsrc = torch.from_numpy(src.view(np.int16) if bits == 16 else src).cuda()
    ddst = torch.zeros_like(dsrc)
    vs.bgr_image_warp_batch_device(dsrc.data_ptr(), n, w, h, 3, bits, [vs.Transform.of(*TRANSFORMS[k]) for k in names], ddst.data_ptr(), mode, border,
                                   max_value=maxv, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = ddst.cpu().numpy()
    return out.view(np.uint16) if bits == 16 else out


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_single_and_batch_entries_equal_the_oracle_twins(gpu_vs, oracle, size, bits):
    import torch
    vs, O = gpu_vs, oracle
    w, h = size
    src = _frames(w, h, bits)
    maxv = 255 if bits == 8 else 1023
    for mode, omode, mname in _modes(vs, O):
        for border, oborder, bname in _borders(vs, O):
            for name in TRANSFORMS:
                want = _want(O, w, h, bits, 0, name, omode, oborder)
                # the single-frame entry (host memory) and a one-frame call of the device batch entry
                got = vs.bgr_image_warp(src[0], vs.Transform.of(*TRANSFORMS[name]), mode=mode, border=border, max_value=maxv)
                assert np.array_equal(got, want), ("single", mname, bname, name)
                got = _device_batch(vs, torch, src[:1], [name], mode, border, maxv)
                assert np.array_equal(got[0], want), ("device batch of 1", mname, bname, name)
            for bn, names in BATCHES.items():
                got = _device_batch(vs, torch, src, names, mode, border, maxv)
                for f, name in enumerate(names):
                    assert np.array_equal(got[f], _want(O, w, h, bits, f, name, omode, oborder)), ("device batch of 5", mname, bname, bn, f, name)


@pytest.mark.parametrize("bits", [8, 10])
def test_window_with_odd_offsets_equals_the_same_cut_of_the_whole_warp(gpu_vs, oracle, bits):
    vs, O = gpu_vs, oracle
    (w, h), roi = ROI_CASE
    rx, ry, rw, rh = roi
    src = _frames(w, h, bits)
    maxv = 255 if bits == 8 else 1023
    for mode, omode, mname in _modes(vs, O):
        for border, oborder, bname in _borders(vs, O):
            for name in TRANSFORMS:
                got = vs.bgr_image_warp_roi_batch(src[:1], [vs.Transform.of(*TRANSFORMS[name])], roi, mode=mode, border=border, max_value=maxv)
                assert np.array_equal(got[0], _want(O, w, h, bits, 0, name, omode, oborder)[ry:ry + rh, rx:rx + rw]), ("window, 1 frame", mname, bname, name)
            for bn, names in BATCHES.items():
                got = vs.bgr_image_warp_roi_batch(src, [vs.Transform.of(*TRANSFORMS[k]) for k in names], roi, mode=mode, border=border, max_value=maxv)
                for f, name in enumerate(names):
                    assert np.array_equal(got[f], _want(O, w, h, bits, f, name, omode, oborder)[ry:ry + rh, rx:rx + rw]), ("window, 5 frames", mname, bname, bn, f, name)
