"""The denoise kernels (vs_denoise.hip) on hostile input: NaN, infinite, singular, near-singular, saturating and quarter-turn maps as later
candidates, samples above the format's maximum, the ghost bound on the device's output under random maps, the C ABI's group seam -- bit for
bit against the rule's restatement (tests/_denoise_ref.py).  Inputs: tests/_hostile_maps.py; every case asserts its premise on the CPU
references before it looks at the GPU.

All kernel-level calls work on DEVICE memory with the destination inside a guard band on all four sides (the host-memory form copies only
the rows' own bytes back)."""
import ctypes as C

import numpy as np
import pytest

import _denoise_ref as R
import _fill_ref as RF
import _hostile_maps as HM

pytestmark = pytest.mark.gpu

G = 3
IDENT = (0.0, 0.0, 0.0, 0.0)
FORMATS = HM.FORMATS


def _dev_denoise(vs, src, cf, maps, fmt, strength=None, ss=None, ds=None, odd=False):
    """vs_bgr_denoise_batch on device memory, the destination frames G rows apart inside a guard-filled buffer -> (n_out, h, w, 3).
    odd: source and destination start one element into their buffers (8-bit: not on a dword -- the per-sample kernel)"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    ss = 3 * w if ss is None else ss
    ds = 3 * w if ds is None else ds
    off = 1 if odd else 0
    host = np.zeros(n_src * h * ss + 8, dtype)
    host[off:off + n_src * h * ss].reshape(n_src, h, ss)[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out, n_cand = idx.shape
    flat = [vs.Transform.of(*t) for row in maps for t in row]
    assert len(flat) == n_out * n_cand
    arr = (vs.Transform * len(flat))(*flat)
    dfs = (h + 2 * G) * ds
    guard = 0x5A if esz == 1 else 0x5A5A
    dhost = np.full(n_out * dfs + 8, guard, dtype)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda())
    dsrc, ddst = as_t(host), as_t(dhost)
    torch.cuda.synchronize()
    p = vs.denoise_params(strength=strength) if strength is not None else None
    vs._check(vs.lib().vs_bgr_denoise_batch(C.c_void_p(dsrc.data_ptr() + off * esz), h * ss, n_src, w, h, ss, fmt, n_out, n_cand,
                                            idx.ctypes.data_as(C.POINTER(C.c_int32)), arr, C.byref(p) if p is not None else None,
                                            C.c_void_p(ddst.data_ptr() + (G * ds + off) * esz), dfs, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    assert (back[:off] == guard).all() and (back[off + n_out * dfs:] == guard).all()
    frames = back[off:off + n_out * dfs].reshape(n_out, h + 2 * G, ds)
    res = frames[:, G:G + h, :3 * w].reshape(n_out, h, w, 3).copy()
    frames[:, G:G + h, :3 * w] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination frame were written"
    assert (frames[:, G + h:] == guard).all(), "rows below a destination frame were written"
    assert (frames[:, G:G + h, 3 * w:] == guard).all(), "the tail of a destination row was written"
    return res


def _ref(O, src, cf, maps, bits, maxv, strength=24):
    with np.errstate(all="ignore"):
        return R.denoise_batch(O, src, cf, [[O.Transform.of(*t) for t in row] for row in maps], bits, maxv, strength)


def _scene(rng, n, w, h, dtype, maxv, amp=5):
    """one blocky picture under fresh noise of +- amp levels per frame"""
    scale = (maxv + 1) // 256
    base = rng.integers(30 * scale, 220 * scale, (h // 8 + 2, w // 8 + 2, 3))
    up = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w]
    return np.clip(up[None] + rng.integers(-amp * scale, amp * scale + 1, (n, h, w, 3)), 0, maxv).astype(dtype)


@pytest.mark.parametrize("shape", [(64, 48), (67, 21)], ids=["64x48", "67x21"])          # (four pixels per lane; the per-sample kernel)
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_hostile_maps_as_later_candidates(gpu_vs, oracle, fmt, shape):
    """each hostile map as candidate 1 between the target and an ordinary candidate 2.  Where the map covers nothing (premise: which maps
    those are, by the rule's int32 coverage -- infinite and huge shifts) the result equals the run without it; where it covers something
    (NaN and singular maps, which put every pixel on source position (0, 0); the near-singular ones; the quarter turns) the rule's samples
    are what the oracle's warp gives there"""
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = shape
    rng = np.random.default_rng(3 * bits + w)
    src = _scene(rng, 4, w, h, dtype, maxv)
    hostile = dict(HM.HOSTILE)
    hostile.update(HM.FILL_EXTREME)
    hostile["row0_trap"] = HM.row0_trap(vs, w, h)
    names = sorted(hostile)
    usual = (0.001, -0.002, 0.4, -0.3)
    maps = [[IDENT, hostile[n], usual] for n in names]
    cf = np.array([[i % 4, (i + 1) % 4, (i + 2) % 4] for i in range(len(maps))], np.int32)
    with np.errstate(all="ignore"):
        covers = {n: bool(RF.covered(O, O.Transform.of(*hostile[n]), w, h).any()) for n in names}
    # (a NaN or singular map does cover: cvRound(NaN) = 0 puts every pixel on source position (0, 0), whose four taps lie in the frame)
    nowhere = {"inf_TX", "inf_both", "ninf_TY", "p1e300", "m1e300", "t_1e300", "tx_6e5", "tx_m3e6", "ty_3e6", "ty_m6e5"}
    assert {n for n in names if not covers[n]} == nowhere and all(covers[n] for n in ("nan_A", "nan_TX", "singular", "near_pp", "row0_trap"))
    want = _ref(O, src, cf, maps, bits, maxv)
    without = _ref(O, src, cf[:, [0, 2]], [[r[0], r[2]] for r in maps], bits, maxv)
    assert (want != src[cf[:, 0]]).mean() > 0.2                      # the ordinary candidate does take part
    for i, n in enumerate(names):
        assert covers[n] or np.array_equal(want[i], without[i]), n
    got = _dev_denoise(vs, src, cf, maps, code)
    bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad
    got = _dev_denoise(vs, src, cf, maps, code, ss=3 * w + 7, ds=3 * w + 5, odd=True)
    bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
    assert not bad, ("unaligned", bad)
    gone = _dev_denoise(vs, src, cf[:, [0, 2]], [[r[0], r[2]] for r in maps], code)
    for i, n in enumerate(names):
        assert covers[n] or np.array_equal(got[i], gone[i]), n


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, oracle, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples of every frame.  Premises: the sampler's saturation
    is live (the result under max_value 65535 differs) and so is the rejection (a target sample of 65535 next to candidates within the
    format lies d >> s >= t away: untouched, above the maximum as it came)"""
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((131, 37), (132, 20)):
        src = _scene(rng, 4, w, h, dtype, maxv)
        for f in src:
            f[rng.random((h, w)) < 0.08] = 65535
            f[rng.random((h, w, 3)) < 0.05] = maxv + 1
        maps = [[IDENT, (0.0, 0.001, 0.3, 0.6), (0.001, 0.0, -0.4, 0.2), (0.0, 0.0, 0.5, 0.5)], [IDENT, (0.0, 0.0, 0.5, 0.5), IDENT, (0.0, 0.0, 1.0, 0.0)]]
        cf = np.array([[0, 1, 2, 3], [3, 2, 1, 0]], np.int32)
        for strength in (24, 255):
            want = _ref(O, src, cf, maps, bits, maxv, strength)
            loose = _ref(O, src, cf, maps, bits, 65535, strength)
            assert not np.array_equal(want, loose)                   # the saturation is live
            tgt = src[cf[:, 0]]
            kept = (tgt == 65535) & (want == 65535)
            assert kept.any() and (want != tgt).mean() > 0.2         # the rejection is live, and so is the blend
            assert want[(want != tgt)].max() <= maxv                 # a blended sample is saturated
            got = _dev_denoise(vs, src, cf, maps, code, strength)
            assert np.array_equal(got, want), (w, h, strength, int((got != want).sum()))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_ghost_bound_on_the_device_output(gpu_vs, oracle, fmt):
    """(c) on uniform noise under random maps, large rotations among them: |out - p| < t << s at every sample of the device's output"""
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(50 + bits)
    for w, h in ((260, 33), (75, 70)):
        src = rng.integers(0, maxv + 1, (5, h, w, 3)).astype(dtype)
        maps = [[IDENT] + [HM._rot(rng, w, h, big=c % 2 == 1) for c in range(4)] for _ in range(3)]
        cf = np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 2, 0, 4, 1]], np.int32)
        for strength in (1, 24, 255):
            want = _ref(O, src, cf, maps, bits, maxv, strength)
            got = _dev_denoise(vs, src, cf, maps, code, strength)
            d = np.abs(got.astype(np.int64) - src[cf[:, 0]].astype(np.int64))
            assert (d < (strength << (bits - 8))).all(), (w, h, strength, int(d.max()))
            assert strength == 1 or d.max() > 0
            assert np.array_equal(got, want)


K_SLOTS = 1 << 15                                                    # the parameter ring's slots (the group sizes)


@pytest.mark.parametrize("n_cand,extra", [(16, 3), (2, 1)])
def test_the_second_group_of_a_long_call(gpu_vs, oracle, n_cand, extra):
    """vs_bgr_denoise_batch uploads candidate entries in groups of (kSlots / 2 / 4) / n_cand output frames: 256 at 16 candidates, 2048 at 2.
    n_out = group + extra crosses the seam: the second group's destination offset and ring span"""
    vs, O = gpu_vs, oracle
    group = (K_SLOTS // 2 // 4) // n_cand
    assert group == {16: 256, 2: 2048}[n_cand]
    n_out = group + extra
    assert n_out > group
    w, h, n_src = 12, 9, 6
    rng = np.random.default_rng(n_cand)
    src = _scene(rng, n_src, w, h, np.uint8, 255)
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    maps = [[(rng.uniform(-0.005, 0.005), rng.uniform(-0.01, 0.01), rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7)) for _ in range(n_cand)] for _ in range(n_out)]
    cf[group - 2:, 1] = (cf[group - 2:, 0] + 1) % n_src              # another frame on both sides of the seam
    want = _ref(O, src, cf, maps, 8, 255)
    assert all((want[o] != src[cf[o, 0]]).any() for o in range(group - 2, n_out))
    got = _dev_denoise(vs, src, cf, maps, vs.FMT_BGR8)
    bad = [o for o in range(n_out) if not np.array_equal(got[o], want[o])]
    assert not bad, (bad[:8], len(bad))
