"""The scene-cut statistics kernel (vs_scene.hip) on hostile input: NaN, infinite, singular, near-singular, saturating and quarter-turn maps,
rint ties on the position, samples above the format's maximum, all-0 against all-maximum frames (the accumulators' extreme) -- bit for bit
against the rule's restatement (tests/_scene_ref.py).  Inputs: tests/_hostile_maps.py; every case asserts its premise on the restatement
before it looks at the GPU.

All calls work on DEVICE memory: the frames lie inside a band of poison on all four sides (a sample read outside a frame would show in sad),
the statistics between guard words, in a buffer filled with poison first -- so the zeroes under the sums are the launcher's."""
import numpy as np
import pytest

import _hostile_maps as HM
import _scene_ref as R

pytestmark = pytest.mark.gpu

G = 3
FORMATS = HM.FORMATS
GUARD64 = 0x5A5A5A5A5A5A5A5A


def _dev_stats(vs, src, pairs, maps, fmt, step=4, poison=None):
    """vs_bgr_scene_stats_batch on device memory -> (n_pairs, 2) uint64.  Frame i lies at rows G .. G + h, columns G .. G + w of a
    (h + 2 G) x (w + 2 G) picture of `poison`; the statistics lie between G guard words a side, over poison"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    esz = src.dtype.itemsize
    poison = (0x5A if esz == 1 else 0x5A5A) if poison is None else poison
    ss = 3 * (w + 2 * G)
    fs = (h + 2 * G) * ss
    host = np.full((n_src, h + 2 * G, ss), poison, src.dtype)
    host[:, G:G + h, 3 * G:3 * G + 3 * w] = src.reshape(n_src, h, 3 * w)
    dsrc = torch.from_numpy(host.view(np.int16) if esz == 2 else host).cuda()
    n_pairs = len(pairs)
    dstats = torch.from_numpy(np.full(2 * n_pairs + 2 * G, GUARD64, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ts = [vs.Transform.of(*t) for t in maps]
    vs.scene_stats_batch_device(dsrc.data_ptr() + (G * ss + 3 * G) * esz, fs, n_src, w, h, ss, fmt, pairs, ts, dstats.data_ptr() + 8 * G,
                                params=vs.scene_params(step=step))
    torch.cuda.synchronize()
    st = dstats.cpu().numpy().view(np.uint64)
    assert (st[:G] == GUARD64).all() and (st[-G:] == GUARD64).all(), "words round the statistics were written"
    assert np.array_equal(dsrc.cpu().numpy().view(src.dtype), host), "the frames were written"
    return st[G:-G].reshape(n_pairs, 2).copy()


def _ref(vs, src, pairs, maps, bits, step=4):
    with np.errstate(all="ignore"):
        return R.stats_batch(vs, src, pairs, [vs.Transform.of(*t) for t in maps], bits, step)


@pytest.mark.parametrize("shape", [(64, 48), (67, 21)], ids=["64x48", "67x21"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_hostile_maps(gpu_vs, fmt, shape):
    """Premises: NaN, infinite, 1e300 and saturating shifts count nothing; singular and near-singular maps and the quarter turns count what the
    restatement counts -- the quarter turns something"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = shape
    rng = np.random.default_rng(3 * bits + w)
    src = rng.integers(0, maxv + 1, (4, h, w, 3)).astype(dtype)
    hostile = dict(HM.HOSTILE)
    hostile.update(HM.FILL_EXTREME)
    hostile["row0_trap"] = HM.row0_trap(vs, w, h)
    names = sorted(hostile)
    maps = [hostile[n] for n in names]
    pairs = [(i % 4, (i + 1) % 4) for i in range(len(maps))]
    for step in (1, 4):
        want = _ref(vs, src, pairs, maps, bits, step)
        counts = {n: int(want[i, 0]) for i, n in enumerate(names)}
        nothing = set(HM.HAS_NAN) | {"p1e300", "m1e300", "t_1e300", "tx_6e5", "tx_m3e6", "ty_3e6", "ty_m6e5"}
        assert all(counts[n] == 0 for n in nothing), counts
        assert any(counts[n] > 0 for n in ("rot90_zoom05", "rot90_zoom2", "rot180_zoom05", "rot180_zoom2"))
        assert R.cuts(want, w, h, step).all()                            # unrelated noise, or no overlap: every pair is a cut
        got = _dev_stats(vs, src, pairs, maps, code, step)
        bad = [names[i] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (step, bad)
        assert np.array_equal(vs.scene_cuts(got, w, h, vs.scene_params(step=step)), R.cuts(want, w, h, step))


@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_rint_ties_on_the_position(gpu_vs, fmt):
    """maps that put every lattice pixel on a tie (tests/_hostile_maps.py's tie_maps: premises asserted there): ties to even names the sample"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    rng = np.random.default_rng(bits)
    for w, h in ((37, 22), (64, 16)):
        src = rng.integers(0, (1 << bits), (3, h, w, 3)).astype(dtype)      # independent noise: a wrong sample shows in sad
        ties = HM.tie_maps(vs, w, h)
        maps = [tr for _, tr in ties]
        pairs = [(i % 3, (i + 1) % 3) for i in range(len(maps))]
        want = _ref(vs, src, pairs, maps, bits, 1)
        assert (want[:, 0] > 0).all()
        # premise: round-half-up would name other samples -- sad differs
        xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
        differ = 0
        for i, tr in enumerate(maps):
            m = np.asarray(HM.cvinv(vs)(vs.Transform.of(*tr), w, h), np.float64)
            qx, qy = np.floor((m[0] * xs + m[1] * ys) + m[2] + 0.5), np.floor((m[3] * xs + m[4] * ys) + m[5] + 0.5)
            ins = (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
            q = src[pairs[i][1]][np.where(ins, qy, 0).astype(int), np.where(ins, qx, 0).astype(int)].astype(np.int64) >> (bits - 8)
            p = src[pairs[i][0]].astype(np.int64) >> (bits - 8)
            differ += int(np.abs(p - q).sum(axis=-1)[ins].sum()) != int(want[i, 1])
        assert differ >= len(maps) - 1
        got = _dev_stats(vs, src, pairs, maps, code, 1)
        bad = [ties[i][0] for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (w, h, bad)


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples of every frame: they count, as the maximum.  Premise: the
    clamp is live -- without it (the raw sample shifted) sad differs"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((131, 37), (132, 20)):
        src = rng.integers(0, maxv + 1, (4, h, w, 3)).astype(dtype)
        for f in src:
            f[rng.random((h, w)) < 0.08] = 65535
            f[rng.random((h, w, 3)) < 0.05] = maxv + 1
        maps = [(0.0, 0.0, 0.0, 0.0), (0.0, 0.001, 0.3, 0.6), (0.0, 0.0, 0.5, 0.5), (0.0, 0.0, 1.0, 0.0)]
        pairs = [(0, 1), (3, 2), (1, 1), (2, 0)]
        want = _ref(vs, src, pairs, maps, bits, 1)
        assert int(want[0, 0]) == w * h and (want[:, 0] > 0).all()
        raw = (np.abs((src[0].astype(np.int64) >> (bits - 8)) - (src[1].astype(np.int64) >> (bits - 8)))).sum()
        assert int(raw) != int(want[0, 1])                               # the clamp is live
        assert np.array_equal(_dev_stats(vs, src, pairs, maps, code, 1), want), (w, h)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_all_zero_against_all_maximum(gpu_vs, fmt):
    """the accumulators' extreme: every counted lattice pixel adds 3 * 255.  257 x 33 at step 1 fills every lane's 32 lattice pixels of the first
    tile (a lane's sad 32 * 765, a wave's 64 times that) and runs into a second tile across and down"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = 257, 33
    top = 65535 if bits > 8 else 255                                   # (above the format's maximum where the container allows: still 255 levels)
    src = np.stack([np.zeros((h, w, 3), dtype), np.full((h, w, 3), top, dtype), np.full((h, w, 3), maxv, dtype)])
    maps = [(0.0, 0.0, 0.0, 0.0)] * 3 + [(0.0, 0.0, 1.0, -1.0)]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0)]
    want = _ref(vs, src, pairs, maps, bits, 1)
    assert want[:3].tolist() == [[w * h, 765 * w * h]] * 3 and want[3].tolist() == [(w - 1) * (h - 1), 765 * (w - 1) * (h - 1)]
    got = _dev_stats(vs, src, pairs, maps, code, 1, poison=0)
    assert np.array_equal(got, want)
    assert vs.scene_cuts(got, w, h, vs.scene_params(step=1, threshold=255)).tolist() == [0, 0, 0, 0]      # 255 levels exactly: equality is no cut
    assert vs.scene_cuts(got, w, h, vs.scene_params(step=1, threshold=254)).tolist() == [1, 1, 1, 1]
