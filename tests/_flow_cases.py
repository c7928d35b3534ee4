"""Hostile inputs for the dense flow (vs_flow.hip), shared by tests/test_flow_cpu.py (what the specification does with them, no GPU)
and tests/test_flow_hostile_gpu.py / test_flow_fill_poison_gpu.py (kernels == specification on them).

Every content class names the property of the SPECIFICATION's result that makes it hostile (`expect`): the CPU test asserts that
property on tests/_flow_ref.py, the GPU test asserts it again before it compares, so a later change of a generator or of the
specification cannot quietly turn a hostile case into a tame one.
"""
import numpy as np

import _flow_ref as R

W, H = 173, 118
TINY = np.float32(np.finfo(np.float32).tiny)          # smallest normal float32


def band_limited(h, w, seed, cutoff=0.05):
    """seeded white noise low-passed by a Gaussian in frequency (periodic), scaled to about 128 +- 40"""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((h, w))
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    t = np.real(np.fft.ifft2(np.fft.fft2(n) * np.exp(-(fx ** 2 + fy ** 2) / (2 * cutoff ** 2))))
    return 128.0 + t / t.std() * 40.0


def u8(a):
    return np.clip(a, 0, 255).round().astype(np.uint8)


def texture_pair(w, h, dx, dy, seed, margin=20):
    """(prev, next) u8 of one band-limited texture, next(x, y) = prev(x - dx, y - dy)"""
    t = band_limited(h + 2 * margin, w + 2 * margin, seed)
    return (u8(t[margin:margin + h, margin:margin + w]), u8(t[margin - dy:margin - dy + h, margin - dx:margin - dx + w]))


def moving_pair(w, h, seed):
    """two u8 frames of a band-limited texture under a small rotation + shift: a smooth, non-constant flow"""
    t = band_limited(h + 64, w + 64, seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = w / 2, h / 2
    ang = 0.01
    sx = np.cos(ang) * (x - cx) - np.sin(ang) * (y - cy) + cx + 32 + 1.7
    sy = np.sin(ang) * (x - cx) + np.cos(ang) * (y - cy) + cy + 32 - 2.3
    return np.clip(t[32:32 + h, 32:32 + w], 0, 255).round().astype(np.uint8), np.clip(sample(t, sx, sy), 0, 255).round().astype(np.uint8)


def sample(t, sx, sy):
    x0 = np.clip(np.floor(sx).astype(np.int64), 0, t.shape[1] - 2)
    y0 = np.clip(np.floor(sy).astype(np.int64), 0, t.shape[0] - 2)
    fx, fy = np.clip(sx - x0, 0, 1), np.clip(sy - y0, 0, 1)
    return (t[y0, x0] * (1 - fx) + t[y0, x0 + 1] * fx) * (1 - fy) + (t[y0 + 1, x0] * (1 - fx) + t[y0 + 1, x0 + 1] * fx) * fy


def _noise(w, h):
    return (np.random.default_rng(101).integers(0, 256, (h, w), dtype=np.uint8),
            np.random.default_rng(202).integers(0, 256, (h, w), dtype=np.uint8))


def _binary(w, h):
    a, b = _noise(w, h)
    return ((a >= 128) * 255).astype(np.uint8), ((b >= 128) * 255).astype(np.uint8)


def _constants(w, h):
    return np.full((h, w), 200, np.uint8), np.full((h, w), 13, np.uint8)


def _checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    a = (((x + y) & 1) * 255).astype(np.uint8)
    return a, (255 - a).astype(np.uint8)


def _one_pixel(w, h):
    a = np.full((h, w), 100, np.uint8)
    b = a.copy()
    b[h // 2, w // 2] = 101
    return a, b


def _ramp(w, h):
    x = np.arange(w)[None, :].repeat(h, 0)
    return (x % 256).astype(np.uint8), ((x + 1) % 256).astype(np.uint8)


def _step(w, h):
    a = np.zeros((h, w), np.uint8)
    b = np.zeros((h, w), np.uint8)
    a[:, w // 2:] = 255
    b[:, w // 2 + 20:] = 255
    return a, b


def _band(w, h):
    return texture_pair(w, h, 3, -2, seed=3)


# name -> (generator(w, h), flow parameters, properties the specification's result must have)
CONTENT = {
    "noise": (_noise, {}, ("finite", "no_zero_magnitude", "beyond_window")),
    "noise_binary": (_binary, {}, ("finite", "beyond_window")),
    "noise_win1": (_noise, dict(winsize=1, iterations=5, levels=1), ("finite", "beyond_frame")),
    "constants": (_constants, {}, ("finite", "one_magnitude")),
    "checkerboard": (_checker, {}, ("finite", "subnormal_flow", "mostly_zero")),
    "one_pixel": (_one_pixel, {}, ("finite", "subnormal_flow", "subnormal_mag2")),
    "ramp": (_ramp, {}, ("finite", "subnormal_mag2", "tiny_median")),
    "step_edge": (_step, {}, ("finite", "beyond_frame", "many_zeros")),
    "band_levels6": (_band, dict(levels=6), ("finite", "wide_blur", "beyond_window")),
}


def content(name, w=W, h=H):
    """(prev, next, parameter overrides, expected properties)"""
    gen, kw, expect = CONTENT[name]
    a, b = gen(w, h)
    return a, b, dict(kw), expect


def subnormal(a):
    a = np.abs(np.asarray(a, np.float32))
    return (a > 0) & (a < TINY)


def mag2(flow):
    return (flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1]).ravel()


def check_property(name, flow, kw):
    """None when the specification's flow has the property, else the reason it has not"""
    m2 = mag2(flow)
    n = m2.size
    h, w = flow.shape[:2]
    p = R.params(**kw)
    if name == "finite":
        return None if np.isfinite(flow).all() else "non-finite flow"
    if name == "no_zero_magnitude":
        return None if np.count_nonzero(m2 == 0) == 0 else "%d zero magnitudes" % np.count_nonzero(m2 == 0)
    if name == "beyond_window":          # motion the window cannot explain: larger than winsize on a layer-0 pixel
        return None if np.abs(flow).max() > p["winsize"] else "max |d| %g" % np.abs(flow).max()
    if name == "beyond_frame":           # x + d far outside the frame: the result lives on update_px's clamp
        return None if np.abs(flow).max() > max(w, h) else "max |d| %g" % np.abs(flow).max()
    if name == "one_magnitude":
        return None if np.unique(m2).size == 1 else "%d distinct magnitudes" % np.unique(m2).size
    if name == "subnormal_flow":
        return None if np.count_nonzero(subnormal(flow)) > 0 else "no subnormal flow component"
    if name == "subnormal_mag2":
        return None if np.count_nonzero(subnormal(m2)) > 0 else "no subnormal squared magnitude"
    if name == "tiny_median":            # element n/2 sits among the smallest normal floats, next to the subnormal ones
        v = np.partition(m2, n // 2)[n // 2]
        return None if 0 < v < 1e-30 else "element n/2 of the squared magnitudes is %g" % v
    if name == "mostly_zero":
        return None if np.count_nonzero(m2 == 0) > n // 2 else "%d zeros of %d" % (np.count_nonzero(m2 == 0), n)
    if name == "many_zeros":
        return None if np.count_nonzero(m2 == 0) > n // 4 else "%d zeros of %d" % (np.count_nonzero(m2 == 0), n)
    if name == "wide_blur":
        r = R.pyr_taps(R.level_geometry(w, h, p["pyr_scale"], p["levels"])[-1][2])[1]
        return None if r > 64 else "top layer's blur radius %d" % r
    raise KeyError(name)


def check_content(name, flow, kw, expect):
    bad = [(e, why) for e in expect for why in [check_property(e, flow, kw)] if why]
    assert not bad, "%s lost its teeth: %r" % (name, bad)


# ---- ties in the selection ---------------------------------------------------------------------------------------------------
def tie_pair(cut, w=W, h=H):
    """the band-limited pair with columns [0, cut) of both frames constant: a run of exactly-zero magnitudes about n/2 long"""
    a, b = texture_pair(w, h, 3, -2, seed=3)
    a, b = a.copy(), b.copy()
    a[:, :cut] = 128
    b[:, :cut] = 128
    return a, b


def zeros_of(cut, w=W, h=H):
    a, b = tie_pair(cut, w, h)
    return int(np.count_nonzero(mag2(R.dense_flow(a, b)) == 0))


def tie_cuts(w=W, h=H):
    """(far below, just below, just above, far above): the cuts `below` leave at most n/2 zero magnitudes (element n/2 is a value past the
    run: the FIRST one past it for `just below`), the cuts `above` more (element n/2 lies inside the run); `just above` is the smallest cut
    whose run reaches past n/2, found by bisection on the specification"""
    lo, hi = 60, w - 20
    zl, zh = zeros_of(lo, w, h), zeros_of(hi, w, h)
    half = (w * h) // 2
    assert zl < half < zh, (zl, zh, half)
    below, above = lo, hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if zeros_of(mid, w, h) > half:
            hi = mid
        else:
            lo = mid
    return below, hi - 1, hi, above


TINY_SHAPES = [(1, 1), (2, 1), (1, 2), (5, 3), (40, 3), (3, 40)]                    # (w, h)
EDGE_SHAPES = [(w, h) for w in (63, 64, 65) for h in (15, 16, 17)]
PARAM_SETS = [dict(winsize=31, poly_n=7, poly_sigma=1.5), dict(winsize=1, poly_n=1, poly_sigma=0.5), dict(winsize=2),
              dict(winsize=16, iterations=1)]


def small_pair(w, h, seed):
    """a moving texture at any size, 1 x 1 included (the margin keeps the texture larger than the motion)"""
    return texture_pair(w, h, 2, -1, seed=seed, margin=8)


def ident(kw):
    return ",".join("%s=%s" % i for i in kw.items()) or "default"
