"""The deflicker kernels (vs_deflicker.hip) on hostile input: NaN, infinite, singular, near-singular, saturating and quarter-turn maps as later
candidates, rint ties on the position, samples above the format's maximum, gains at both clamps and beyond them, caller-made statistics at the
sums' bound and on the divisions' ties -- bit for bit against the rule's restatement (tests/_deflicker_ref.py).  Inputs: tests/_hostile_maps.py;
every case asserts its premise on the CPU reference before it looks at the GPU.

All kernel-level calls work on DEVICE memory with the destination, the statistics and the gains inside guard bands."""
import numpy as np
import pytest

import _deflicker_ref as R
import _hostile_maps as HM

pytestmark = pytest.mark.gpu

G = 3
IDENT = (0.0, 0.0, 0.0, 0.0)
FORMATS = HM.FORMATS
UNIT = 32768
GUARD64, GUARD32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def _as_t(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _dev_stats(vs, src, cf, maps, fmt, step=4, ss=None, odd=False):
    """vs_bgr_exposure_stats_batch and vs_exposure_gains_batch on device memory, statistics and gains inside guard words -> (stats, gains)"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    esz = src.dtype.itemsize
    ss = 3 * w if ss is None else ss
    off = 1 if odd else 0
    host = np.zeros(n_src * h * ss + 8, src.dtype)
    host[off:off + n_src * h * ss].reshape(n_src, h, ss)[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out, n_cand = idx.shape
    ct = [[vs.Transform.of(*t) for t in row] for row in maps]
    dsrc = _as_t(host)
    dstats = torch.from_numpy(np.full(n_out * n_cand * 8 + 2 * G, GUARD64, np.uint64).view(np.int64)).cuda()
    dgains = torch.from_numpy(np.full(n_out * 4 + 2 * G, GUARD32, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    p = vs.deflicker_params(step=step)
    vs.exposure_stats_batch_device(dsrc.data_ptr() + off * esz, h * ss, n_src, w, h, ss, fmt, idx, ct, dstats.data_ptr() + 8 * G, params=p)
    vs.exposure_gains_batch_device(dstats.data_ptr() + 8 * G, n_out, n_cand, w, h, dgains.data_ptr() + 4 * G, params=p)
    torch.cuda.synchronize()
    st = dstats.cpu().numpy().view(np.uint64)
    gg = dgains.cpu().numpy().view(np.uint32)
    assert (st[:G] == GUARD64).all() and (st[-G:] == GUARD64).all(), "words round the statistics were written"
    assert (gg[:G] == GUARD32).all() and (gg[-G:] == GUARD32).all(), "words round the gains were written"
    return st[G:-G].reshape(n_out, n_cand, 8).copy(), gg[G:-G].reshape(n_out, 4).copy()


def _dev_gains_of(vs, stats, w, h, step=4):
    """vs_exposure_gains_batch on caller-made statistics in device memory"""
    import torch
    stats = np.ascontiguousarray(stats, np.uint64)
    n_out, n_cand = stats.shape[:2]
    dstats = torch.from_numpy(stats.view(np.int64)).cuda()
    dgains = torch.from_numpy(np.full(n_out * 4 + 2 * G, GUARD32, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    vs.exposure_gains_batch_device(dstats.data_ptr(), n_out, n_cand, w, h, dgains.data_ptr() + 4 * G, params=vs.deflicker_params(step=step))
    torch.cuda.synchronize()
    gg = dgains.cpu().numpy().view(np.uint32)
    assert (gg[:G] == GUARD32).all() and (gg[-G:] == GUARD32).all()
    return gg[G:-G].reshape(n_out, 4).copy()


def _dev_gain(vs, src, gains, fmt, ss=None, ds=None, odd=False, in_place=False):
    """vs_bgr_gain_batch on device memory with the gains in device memory (the host never sees them: the kernel clamps), the destination frames G
    rows apart inside a guard-filled buffer -> (n, h, w, 3)"""
    import torch
    src = np.ascontiguousarray(src)
    n, h, w, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    ss = 3 * w if ss is None else ss
    ds = 3 * w if ds is None else ds
    off = 1 if odd else 0
    guard = 0x5A if esz == 1 else 0x5A5A
    if in_place:
        ss = ds
    dfs = (h + 2 * G) * ds
    dhost = np.full(n * dfs + 8, guard, dtype)
    dgains = torch.from_numpy(np.ascontiguousarray(gains, np.uint32).view(np.int32)).cuda()
    if in_place:
        dhost[off:off + n * dfs].reshape(n, h + 2 * G, ds)[:, G:G + h, :3 * w] = src.reshape(n, h, 3 * w)
        ddst = _as_t(dhost)
        sptr, sfs = ddst.data_ptr() + (G * ds + off) * esz, dfs
    else:
        host = np.zeros(n * h * ss + 8, dtype)
        host[off:off + n * h * ss].reshape(n, h, ss)[:, :, :3 * w] = src.reshape(n, h, 3 * w)
        dsrc, ddst = _as_t(host), _as_t(dhost)
        sptr, sfs = dsrc.data_ptr() + off * esz, h * ss
    torch.cuda.synchronize()
    vs.bgr_gain_batch_device(sptr, sfs, n, w, h, ss, fmt, dgains.data_ptr(), ddst.data_ptr() + (G * ds + off) * esz, dfs, ds)
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    assert (back[:off] == guard).all() and (back[off + n * dfs:] == guard).all()
    frames = back[off:off + n * dfs].reshape(n, h + 2 * G, ds)
    res = frames[:, G:G + h, :3 * w].reshape(n, h, w, 3).copy()
    frames[:, G:G + h, :3 * w] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination frame were written"
    assert (frames[:, G + h:] == guard).all(), "rows below a destination frame were written"
    assert (frames[:, G:G + h, 3 * w:] == guard).all(), "the tail of a destination row was written"
    return res


def _ref(O, src, cf, maps, bits, step=4):
    with np.errstate(all="ignore"):
        return R.stats_batch(O, src, cf, [[O.Transform.of(*t) for t in row] for row in maps], bits, step)


def _scene(rng, n, w, h, dtype, maxv, amp=5):
    """one blocky picture under fresh noise, frame i at exposure 0.8 + 0.1 i; every level counted"""
    scale = (maxv + 1) // 256
    base = rng.integers(40 * scale, 150 * scale, (h // 8 + 2, w // 8 + 2, 3))
    up = np.repeat(np.repeat(base, 8, 0), 8, 1)[:h, :w]
    f = (up[None] + rng.integers(-amp * scale, amp * scale + 1, (n, h, w, 3))) * (0.8 + 0.1 * np.arange(n))[:, None, None, None]
    return np.clip(np.floor(f), scale, 254 * scale).astype(dtype)


@pytest.mark.parametrize("shape", [(64, 48), (67, 21)], ids=["64x48", "67x21"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_hostile_maps_as_later_candidates(gpu_vs, oracle, fmt, shape):
    """each hostile map as candidate 1 between the target and an ordinary candidate 2.  Premises: NaN, infinite, 1e300 and saturating shifts count
    nothing; singular and near-singular maps and the quarter turns count what the restatement counts -- the quarter turns something"""
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
    for step in (1, 4):
        want = _ref(O, src, cf, maps, bits, step)
        counts = {n: int(want[i, 1, 0]) for i, n in enumerate(names)}
        nothing = set(HM.HAS_NAN) | {"p1e300", "m1e300", "t_1e300", "tx_6e5", "tx_m3e6", "ty_3e6", "ty_m6e5"}
        assert all(counts[n] == 0 for n in nothing), counts
        assert any(counts[n] > 0 for n in ("rot90_zoom05", "rot90_zoom2", "rot180_zoom05", "rot180_zoom2"))
        assert (want[:, 2, 0] > 0).all()                             # the ordinary candidate does count
        got, gains = _dev_stats(vs, src, cf, maps, code, step)
        bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (step, bad)
        assert np.array_equal(gains, R.gains_batch(want, w, h, step))
        got, _ = _dev_stats(vs, src, cf, maps, code, step, ss=3 * w + 7, odd=True)
        bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, ("unaligned", step, bad)


@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_rint_ties_on_the_position(gpu_vs, oracle, fmt):
    """maps that put every lattice pixel on a tie (tests/_hostile_maps.py's tie_maps: premises asserted there): ties to even names the sample"""
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((37, 22), (64, 16)):
        src = rng.integers(1 << (bits - 8), 255 << (bits - 8), (3, h, w, 3)).astype(dtype)      # independent noise: a wrong sample shows in the sums
        ties = HM.tie_maps(vs, w, h)
        maps = [[IDENT, tr, IDENT] for _, tr in ties]
        cf = np.array([[i % 3, (i + 1) % 3, (i + 2) % 3] for i in range(len(maps))], np.int32)
        want = _ref(O, src, cf, maps, bits, 1)
        assert (want[:, 1, 0] > 0).all()
        # premise: round-half-up would name other samples -- the sums differ
        M = [np.asarray(HM.cvinv(vs)(vs.Transform.of(*tr), w, h), np.float64) for _, tr in ties]
        xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
        differ = 0
        for i, m in enumerate(M):
            qx, qy = np.floor((m[0] * xs + m[1] * ys) + m[2] + 0.5), np.floor((m[3] * xs + m[4] * ys) + m[5] + 0.5)
            ins = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
            q = src[cf[i, 1]][np.where(ins, qy, 0).astype(int), np.where(ins, qx, 0).astype(int)].astype(np.int64)
            differ += int(q[..., 0][ins].sum()) != int(want[i, 1, 4])
        assert differ >= len(M) - 1
        got, _ = _dev_stats(vs, src, cf, maps, code, 1)
        bad = [ties[i][0] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (w, h, bad)


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, oracle, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples of every frame.  Premises: the rejection is live (fewer
    pairs count than without those samples, and no sum holds one) and so is the gain pass's saturation (the result under max_value 65535
    differs); an out-of-range sample of a frame with unit gains comes back as it is"""
    vs, O = gpu_vs, oracle
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((131, 37), (132, 20)):
        clean = _scene(rng, 4, w, h, dtype, maxv)
        src = clean.copy()
        for f in src:
            f[rng.random((h, w)) < 0.08] = 65535
            f[rng.random((h, w, 3)) < 0.05] = maxv + 1
        maps = [[IDENT, (0.0, 0.001, 0.3, 0.6), (0.001, 0.0, -0.4, 0.2), (0.0, 0.0, 0.5, 0.5)], [IDENT, (0.0, 0.0, 0.5, 0.5), IDENT, (0.0, 0.0, 1.0, 0.0)],
                [IDENT, (0.0, 0.0, 900.0, 0.0), (0.0, 0.0, 0.0, 900.0), (0.0, 0.0, -900.0, 0.0)]]
        cf = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 2, 3, 0]], np.int32)
        want = _ref(O, src, cf, maps, bits, 1)
        full = _ref(O, clean, cf, maps, bits, 1)
        assert (want[:2, 1:, 0] < full[:2, 1:, 0]).all() and (want[:2, 1:, 0] > 0).all()
        assert (want[:, :, 1:7] <= want[:, :, :1] * ((255 << (bits - 8)) - 1)).all()              # no sum holds a rejected sample
        got, gains = _dev_stats(vs, src, cf, maps, code, 1)
        assert np.array_equal(got, want), (w, h)
        want_g = R.gains_batch(want, w, h, 1)
        assert np.array_equal(gains, want_g) and (want_g[2, :3] == UNIT).all() and (want_g[:2, :3] != UNIT).all()
        tgt = src[cf[:, 0]]
        out = R.gain_batch(tgt, want_g, maxv)
        assert not np.array_equal(out[:2], R.gain_batch(tgt[:2], want_g[:2], 65535))              # the saturation is live
        assert out[:2].max() == maxv and np.array_equal(out[2], tgt[2]) and tgt[2].max() == 65535
        for kw in (dict(), dict(ss=3 * w + 7, ds=3 * w + 5, odd=True), dict(in_place=True), dict(in_place=True, ds=3 * w + 3, odd=True)):
            res = _dev_gain(vs, tgt, gains, code, **kw)
            assert np.array_equal(res, out), (w, h, kw, int((res != out).sum()))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_gains_at_both_clamps_and_beyond(gpu_vs, fmt):
    """the gain pass at 16384 and 65536, and with gains in device memory outside that range: the kernel clamps them (a host-memory gain out of
    range is refused: tests/test_deflicker_gpu.py).  Uniform noise over the whole container"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(70 + bits)
    for w, h in ((260, 33), (75, 18)):
        src = rng.integers(0, (255 if bits == 8 else 65535) + 1, (6, h, w, 3)).astype(dtype)
        inside = np.array([[16384, 65536, UNIT, 0], [65536, 16384, 16385, 0], [UNIT, UNIT, UNIT, 7], [UNIT, UNIT, 32769, 0], [40000, 20000, 65535, 0],
                           [65536, 65536, 65536, 0]], np.uint32)
        beyond = np.array([[0, 0xFFFFFFFF, UNIT, 0], [65537, 16383, 16385, 0], [UNIT, UNIT, UNIT, 7], [UNIT, UNIT, 32769, 0], [40000, 20000, 65535, 0],
                           [1 << 31, 70000, 1 << 17, 0]], np.uint32)
        want = R.gain_batch(src, inside, maxv)
        assert np.array_equal(want[2], src[2]) and want[5].max() == maxv and (want[0][..., 0] <= (src[0][..., 0].astype(np.int64) + 1) // 2).all()
        for kw in (dict(), dict(ss=3 * w + 1, ds=3 * w + 3), dict(in_place=True), dict(odd=True)):
            assert np.array_equal(_dev_gain(vs, src, inside, code, **kw), want), (w, h, kw)
            assert np.array_equal(_dev_gain(vs, src, beyond, code, **kw), want), ("beyond", w, h, kw)


def test_caller_made_statistics_at_the_bound_and_on_the_ties(gpu_vs):
    """vs_exposure_gains_batch on statistics no frame produced: sums of 2^46 - 1 (every term of the ratio below 2^63), the two divisions' ties, the
    clamps, count at and one below max(1, L / 16), a_c == 0 under a used count"""
    vs = gpu_vs
    w, h, step = 64, 64, 4
    thr = R.threshold(w, h, step)
    big = 2 ** 46 - 1
    z = [0] * 8
    rows = [
        [z, [thr, big, big, big, big, big, big, 0], z],
        [z, [2 ** 30 - 1, 1, 1, 1, big, big, big, 0], [thr, big, big, big, 1, 1, 1, 0]],
        [z, [thr, 65536, 65536, 65536, 65537, 65537, 65537, 0], z],                       # r on its tie, G on its tie (m = 1)
        [z, [thr, 65536, 65536, 65536, 65537, 65537, 65537, 0], [thr, 65536, 65536, 65536, 65537, 65537, 65537, 0]],
        [z, [thr - 1, 100, 100, 100, 200, 200, 200, 0], [thr, 100, 100, 100, 200, 200, 200, 0]],
        [z, [thr, 0, 5, 0, 7, 7, 7, 0], z],                                               # a_c == 0: r = 32768 there
        [z, [thr, big, 3, big - 1, big - 1, big, 2, 0], [thr, 256, 256, 256, 257, 257, 257, 0]],
    ]
    stats = np.array(rows, np.uint64)
    want = R.gains_batch(stats, w, h, step)
    assert want[0].tolist() == [UNIT, UNIT, UNIT, 1] and want[1].tolist() == [(2 * (UNIT + 65536 + 16384) + 3) // 6] * 3 + [2]
    assert want[2].tolist() == [32769, 32769, 32769, 1] and want[3].tolist() == [32769, 32769, 32769, 2]
    assert want[4].tolist() == [49152, 49152, 49152, 1] and want[5].tolist() == [UNIT, (2 * (UNIT + 45875) + 2) // 4, UNIT, 1]
    assert ((want[:, :3] >= 16384) & (want[:, :3] <= 65536)).all()
    assert np.array_equal(_dev_gains_of(vs, stats, w, h, step), want)
    assert np.array_equal(vs.exposure_gains_batch(stats, w, h, params=vs.deflicker_params(step=step)), want)
    # beyond the bounds, in device memory: the arithmetic wraps, nothing faults, the gains keep their range
    wild = np.array([[z, [2 ** 40, 2 ** 63, 2 ** 64 - 1, 2 ** 50, 2 ** 64 - 1, 2 ** 63, 2 ** 47, 0], [1, 2 ** 64 - 1, 1, 0, 3, 2 ** 64 - 1, 2 ** 64 - 1, 0]]], np.uint64)
    g = _dev_gains_of(vs, wild, w, h, step)
    assert ((g[:, :3] >= 16384) & (g[:, :3] <= 65536)).all() and g[0, 3] == 1
