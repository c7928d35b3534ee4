"""The scene-cut statistics on the GPU (include/vs_amd.h: vs_bgr_scene_stats_batch) against the rule's restatement (tests/_scene_ref.py):
np.array_equal -- the rule fixes every bit, and the sums are integers.  Every case asserts its premise on the restatement before it looks at the
GPU."""
import numpy as np
import pytest

import _scene_ref as R

pytestmark = pytest.mark.gpu

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr16": (4, np.uint16, 16)}
# (w, h, step).  Frames smaller than a wave (1 x 1, 3 x 2, 63 x 5, 65 x 33); a lattice of 257 columns, one past the wave's four 64-column chunks,
# once at step 1 and once at step 4; a lattice of 33 rows, one past a workgroup's four 8-row strips (65 x 33 at step 1, 9 x 129 at step 4);
# steps 1, 3, 4 and 64 (64: a lattice of 2 x 1 and of 1 x 1)
SHAPES = [(1, 1, 1), (1, 1, 64), (3, 2, 1), (3, 2, 3), (63, 5, 1), (63, 5, 4), (65, 33, 1), (65, 33, 3), (65, 33, 64), (257, 9, 1), (1025, 9, 4), (9, 129, 4),
          (130, 70, 64)]


def _frames(rng, n, w, h, dtype, maxv):
    """one picture under fresh noise per frame, frame i a little brighter than frame i - 1; the full range occurs, black and clipped samples too"""
    yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
    base = ((xx * 5 + yy * 3 + 40 * cc) % 256) * ((maxv + 1) // 256)
    f = base[None] + rng.integers(-(maxv // 16), maxv // 16 + 1, (n, h, w, 3)) + (np.arange(n) * (maxv // 40))[:, None, None, None]
    return np.clip(f, 0, maxv).astype(dtype)


def _transforms(vs, w, h):
    """identity; whole-pixel shifts; half-pixel shifts, where rint's ties decide (0.5 -> 0, 1.5 -> 2); a rotation with zoom; a map off the frame"""
    T = vs.Transform.of
    return [T(), T(0, 0, 1, 0), T(0, 0, -2, 1), T(0, 0, 0.5, 0.5), T(0, 0, -1.5, 2.5), T(0.03, 0.05, 1.25, -0.75), T(-0.02, -0.04, -0.5, 0.25),
            T(0, 0, 3.0 * w + 7, 0)]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_statistics_equal_the_rule(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(100 + bits)
    counted = ties = 0
    for w, h, step in SHAPES:
        src = _frames(rng, 3, w, h, dtype, maxv)
        ts = _transforms(vs, w, h)
        # pairs out of order, the same frame twice, every transform once
        pairs = [(k % 3, (2 * k + 1) % 3) for k in range(len(ts))]
        pairs[0] = (2, 2)
        p = vs.scene_params(step=step)
        want = R.stats_batch(vs, src, pairs, ts, bits, step)
        assert want[0].tolist() == [R.lattice_size(w, h, step), 0]      # premise: a frame against itself under the identity
        assert want[-1].tolist() == [0, 0]                               # ... and a map off the frame
        counted += int(want[:, 0].sum())
        qx, _, inside = R.pair_positions(vs, ts[3], w, h, step)
        ties += int(inside.sum())
        got = vs.scene_stats_batch(src, pairs, ts, params=p, fmt=code)
        assert np.array_equal(got, want), (w, h, step, got.tolist(), want.tolist())
        # pitched rows, odd and on dwords
        for ss in (3 * w + 7, 3 * w + 8):
            assert np.array_equal(vs.scene_stats_batch(src, pairs, ts, params=p, fmt=code, src_stride=ss), want), (w, h, step, ss)
    assert counted > 20000 and ties > 5000                               # the comparison was about counted pairs, half-pixel ones among them


def test_half_pixel_ties_go_to_even(gpu_vs):
    """x - 0.5 for x = 0, 1, 2, 3 is -0.5, 0.5, 1.5, 2.5 -> -0 (inside), 0, 2, 2: a column ramp shows which sample was taken"""
    vs = gpu_vs
    w, h = 8, 2
    ramp = np.zeros((h, w, 3), np.uint8)
    ramp[:, :, :] = (np.arange(w) * 10)[None, :, None]
    src = np.stack([np.zeros_like(ramp), ramp])
    t = vs.Transform.of(0, 0, 0.5, 0)
    assert vs.cv_inverse_matrix(t, w, h)[2] == -0.5
    want = R.pair_stats(vs, src[0], src[1], t, 8, 1)
    assert want == [2 * 8, 2 * 3 * 10 * (0 + 0 + 2 + 2 + 4 + 4 + 6 + 6)]
    assert vs.scene_stats_batch(src, [(0, 1)], [t], params=vs.scene_params(step=1)).tolist() == [want]


def test_the_three_consequences_and_defaults(gpu_vs):
    vs = gpu_vs
    T = vs.Transform.of
    rng = np.random.default_rng(5)
    w, h = 260, 75
    a = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    b = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    b[:h - 2, :w - 3] = a[2:, 3:]
    lo, hi = np.full((h, w, 3), 100, np.uint8), np.full((h, w, 3), 130, np.uint8)
    src = np.stack([a, b, lo, hi])
    L = R.lattice_size(w, h, 4)
    got = vs.scene_stats_batch(src, [(0, 0), (0, 1), (2, 3), (3, 2)], [T(), T(0, 0, 3, 2), T(), T()])      # NULL parameters: step 4
    overlap = len(range(4, w, 4)) * len(range(4, h, 4))
    assert got.tolist() == [[L, 0], [overlap, 0], [L, 90 * L], [L, 90 * L]]
    assert vs.scene_cuts(got, w, h).tolist() == [0, 0, 0, 0]             # 30 levels: under the default threshold
    assert vs.scene_cuts(got, w, h, vs.scene_params(threshold=29)).tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("n_pairs", [0, 1, 70])
def test_pair_counts(gpu_vs, n_pairs):
    """70 pairs on 8 x 5 frames: more than a kernel-argument block carries"""
    vs = gpu_vs
    rng = np.random.default_rng(70 + n_pairs)
    w, h, n_src = 8, 5, 6
    src = _frames(rng, n_src, w, h, np.uint8, 255)
    pairs = [(int(rng.integers(0, n_src)), int(rng.integers(0, n_src))) for _ in range(n_pairs)]
    ts = [vs.Transform.of(0, 0, *rng.uniform(-2.5, 2.5, 2)) for _ in range(n_pairs)]
    want = R.stats_batch(vs, src, pairs, ts, 8, 1)
    got = vs.scene_stats_batch(src, pairs, ts, params=vs.scene_params(step=1))
    assert got.shape == (n_pairs, 2) and np.array_equal(got, want)
    if n_pairs == 70:
        assert want[:, 0].min() > 0 and len({tuple(r) for r in want.tolist()}) > 60


@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_device_memory_and_unaligned_frames(gpu_vs, fmt):
    """device memory, enqueue only: dense frames on dwords, and frames that start one element into their buffer with an odd pitch; the statistics
    land between two guard words that stay as they were"""
    import torch
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(9 + bits)
    w, h, n_src = 132, 50, 5
    src = _frames(rng, n_src, w, h, dtype, maxv)
    ts = _transforms(vs, w, h) * 5
    pairs = [(int(rng.integers(0, n_src)), int(rng.integers(0, n_src))) for _ in ts]
    want = R.stats_batch(vs, src, pairs, ts, bits, 4)
    assert (want[:, 0] > 0).sum() > 30
    guard = 0x5A5A5A5A5A5A5A5A
    for off, ss in ((0, 3 * w), (1, 3 * w + 7)):
        host = np.zeros(n_src * h * ss + 8, dtype)
        host[off:off + n_src * h * ss].reshape(n_src, h, ss)[:, :, :3 * w] = src.reshape(n_src, h, 3 * w)
        dsrc = torch.from_numpy(host.view(np.int16) if esz == 2 else host).cuda()
        dstats = torch.full((2 * len(ts) + 2,), guard, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        vs.scene_stats_batch_device(dsrc.data_ptr() + off * esz, h * ss, n_src, w, h, ss, code, pairs, ts, dstats.data_ptr() + 8)
        torch.cuda.synchronize()
        got = dstats.cpu().numpy().view(np.uint64)
        assert got[0] == guard and got[-1] == guard
        assert np.array_equal(got[1:-1].reshape(-1, 2), want), (off, ss)
