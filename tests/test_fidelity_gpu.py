"""The fidelity statistics on the GPU (include/vs_amd.h: vs_bgr_fidelity_batch; the kernel: vs_fidelity.hip) against the rule's restatement
(tests/_fidelity_ref.py): np.array_equal -- the rule fixes every bit, and the sums are integers.  The shapes sit on both sides of every seam of the
kernel's tiling, which are read from its constants."""
import os

import numpy as np
import pytest

import _fidelity_ref as R
from _diff import same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMATS = {"bgr8": (1, np.uint8, 8), "bgr10": (2, np.uint16, 10), "bgr12": (3, np.uint16, 12), "bgr16": (4, np.uint16, 16)}


# the seams of vs_fidelity.hip's tiling, in pixels: FD_STRIP_PX (a wave's strip advances by that many columns), FD_BAND_PX (a wave's row band),
# FD_TILE_PX (a workgroup's rows); test_the_seams_are_the_kernel_s holds them against the kernel's constants
STRIP, BAND, TILE = 252, 64, 256
SMALL = [(1, 1), (7, 9), (8, 8), (11, 8), (12, 12), (9, 1025)]
# one less than, at, one more and four more than each seam: the strip (a window needs the next four columns too), the band, the workgroup's tile;
# then both at once, and two strips by two bands
SEAMS = [(STRIP + d, 9) for d in (-1, 0, 1, 4)] + [(STRIP + 4 + d, 12) for d in (-1, 0, 1, 4)] + [(9, BAND + d) for d in (-1, 0, 1, 4)] + \
        [(12, TILE + d) for d in (-1, 0, 1, 4)] + [(STRIP + 1, BAND + 1), (2 * STRIP + 5, 2 * BAND + 3)]


def test_the_seams_are_the_kernel_s():
    """the kernel's constants as its source states them: a change there fails here, and the shapes above are revisited"""
    text = open(os.path.join(ROOT, "video_stabilizer_amd", "csrc", "vs_fidelity.hip")).read()
    assert "constexpr int FD_COLS = 63, FD_BAND = 16, FD_WAVES = 4;" in text
    assert "constexpr int FD_STRIP_PX = 4 * FD_COLS, FD_BAND_PX = 4 * FD_BAND, FD_TILE_PX = FD_BAND_PX * FD_WAVES;" in text
    assert (STRIP, BAND, TILE) == (4 * 63, 4 * 16, 4 * 16 * 4)


def _frames(rng, n, w, h, dtype, maxv):
    """one picture under fresh noise per frame, frame i a little brighter than frame i - 1: the pairs are alike, as consecutive frames are; the
    full range occurs, black and clipped samples too"""
    yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
    base = ((xx * 5 + yy * 3 + 40 * cc) % 256) * ((maxv + 1) // 256)
    f = base[None] + rng.integers(-(maxv // 16), maxv // 16 + 1, (n, h, w, 3)) + (np.arange(n) * (maxv // 40))[:, None, None, None]
    return np.clip(f, 0, maxv).astype(dtype)


def _on_dwords_stride(w):
    return (3 * w + 3) // 4 * 4 + 4


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_statistics_equal_the_rule(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(200 + bits)
    windows = 0
    for w, h in SMALL + SEAMS:
        a = _frames(rng, 3, w, h, dtype, maxv)
        b = _frames(rng, 2, w, h, dtype, maxv)
        pairs = [(2, 1), (0, 0), (1, 1), (2, 1), (0, 1)]                # out of order, one repeated
        want = R.stats_batch(a, b, pairs, bits)
        nwx, nwy = R.n_windows(w, h)
        assert (want[:, 4] == nwx * nwy).all() and (want[:, :3].sum(axis=1) > 0).all()
        windows += nwx * nwy
        got = vs.fidelity_stats_batch(a, b, pairs, fmt=code)
        assert np.array_equal(got, want), (w, h, got.tolist(), want.tolist())
        # pitched rows: odd (no row on a dword but the first) and on dwords, the two sides apart
        for sa, sb in ((3 * w + 7, _on_dwords_stride(w)), (_on_dwords_stride(w), _on_dwords_stride(w) + 4)):
            got = vs.fidelity_stats_batch(a, b, pairs, fmt=code, a_stride=sa, b_stride=sb)
            assert np.array_equal(got, want), (w, h, sa, sb, got.tolist(), want.tolist())
        # one batch on both sides, an image against itself among the pairs
        pairs1 = [(0, 1), (2, 2), (1, 0), (2, 0)]
        want1 = R.stats_batch(a, a, pairs1, bits)
        assert want1[1].tolist() == [0, 0, 0, 0, nwx * nwy, 65536 * nwx * nwy] and np.array_equal(want1[0], want1[2])
        for ss in (None, _on_dwords_stride(w)):
            assert np.array_equal(vs.fidelity_stats_batch(a, None, pairs1, fmt=code, a_stride=ss), want1), (w, h, ss)
    assert windows > 1000


@pytest.mark.parametrize("fmt", ["bgr8", "bgr12"])
def test_a_window_of_a_larger_frame(gpu_vs, fmt):
    """the image is a window of the frame, handed over as its origin pointer with the frame's strides: an origin at an odd pixel of an odd row (no row
    of the window starts on a dword), and one that keeps the rows on dwords"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(300 + bits)
    fw, fh = STRIP + 20, BAND + 14
    a = _frames(rng, 3, fw, fh, dtype, maxv)
    b = _frames(rng, 3, fw, fh, dtype, maxv)
    pairs = [(0, 2), (1, 1), (2, 0)]
    for x, y, rw, rh, ss in ((1, 1, STRIP + 9, BAND + 5, None), (3, 5, 37, 21, None), (4, 3, STRIP + 9, BAND + 5, _on_dwords_stride(fw)),
                             (8, 1, STRIP + 4, BAND + 1, _on_dwords_stride(fw))):
        want = R.stats_batch(a[:, y:y + rh, x:x + rw], b[:, y:y + rh, x:x + rw], pairs, bits)
        assert (want[:, 4] > 0).all()
        got = vs.fidelity_stats_batch(a, b, pairs, fmt=code, a_stride=ss, b_stride=ss, roi=(x, y, rw, rh))
        assert np.array_equal(got, want), (x, y, rw, rh, got.tolist(), want.tolist())


@pytest.mark.parametrize("n_pairs", [0, 1, 70])
def test_pair_counts(gpu_vs, n_pairs):
    """70 pairs: more than a kernel-argument block carries; repeated pairs, any order, images against themselves"""
    vs = gpu_vs
    rng = np.random.default_rng(70 + n_pairs)
    w, h, n_a, n_b = 13, 10, 6, 4
    a = _frames(rng, n_a, w, h, np.uint8, 255)
    b = np.concatenate([a[:2], _frames(rng, n_b - 2, w, h, np.uint8, 255)])
    pairs = [(int(rng.integers(0, n_a)), int(rng.integers(0, n_b))) for _ in range(n_pairs)]
    want = R.stats_batch(a, b, pairs, 8)
    got = vs.fidelity_stats_batch(a, b, pairs)
    assert got.shape == (n_pairs, 6) and same(got, want)
    if n_pairs == 70:
        assert len(set(pairs)) < 70 and len({tuple(r) for r in want.tolist()}) > 15 and (want[:, 0] == 0).any()


@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_device_memory(gpu_vs, fmt):
    """device memory, enqueue only: dense frames on dwords, and frames that start one element into their buffer with an odd pitch; one batch and two;
    the statistics land between two guard words that stay as they were"""
    import torch
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    esz = np.dtype(dtype).itemsize
    rng = np.random.default_rng(9 + bits)
    w, h, n = STRIP + 8, BAND + 6, 4
    a = _frames(rng, n, w, h, dtype, maxv)
    b = _frames(rng, n, w, h, dtype, maxv)
    pairs = [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(9)] + [(3, 3)]
    want2, want1 = R.stats_batch(a, b, pairs, bits), R.stats_batch(a, a, pairs, bits)
    guard = 0x5A5A5A5A5A5A5A5A

    def upload(frames, off, ss):
        host = np.zeros(n * h * ss + 8, dtype)
        host[off:off + n * h * ss].reshape(n, h, ss)[:, :, :3 * w] = frames.reshape(n, h, 3 * w)
        return torch.from_numpy(host.view(np.int16) if esz == 2 else host).cuda()
    for off, ss in ((0, 3 * w), (1, 3 * w + 7)):
        da, db = upload(a, off, ss), upload(b, off, ss)
        for other, want in ((db, want2), (da, want1)):
            dstats = torch.full((6 * len(pairs) + 2,), guard, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            vs.fidelity_stats_batch_device(da.data_ptr() + off * esz, h * ss, n, ss, other.data_ptr() + off * esz, h * ss, n, ss, w, h, code, pairs,
                                           dstats.data_ptr() + 8)
            torch.cuda.synchronize()
            got = dstats.cpu().numpy().view(np.uint64)
            assert got[0] == guard and got[-1] == guard
            assert same(got[1:-1].reshape(-1, 6), want), (off, ss)


def test_more_pairs_than_one_launch_takes(gpu_vs):
    """65 537 pairs of 8 x 8 images: more than the 65 535 a launch's grid z takes.  The pairs' entries travel in groups of half the parameter ring
    (16 384 pairs), each a launch of its own with the entries and the statistics offset by the group's first pair, so what this crosses is the
    GROUP seam, four times; the launcher's own grid-z chunking behind it is a guard that no caller reaches and no test runs"""
    vs = gpu_vs
    rng = np.random.default_rng(65537)
    a = _frames(rng, 7, 8, 8, np.uint8, 255)
    b = _frames(rng, 5, 8, 8, np.uint8, 255)
    pairs = np.stack([rng.integers(0, 7, 65537), rng.integers(0, 5, 65537)], axis=1)
    want = R.stats_batch(a, b, pairs, 8)
    assert (want[:, 4] == 1).all() and len({tuple(r) for r in want.tolist()}) == 35
    got = vs.fidelity_stats_batch(a, b, pairs)
    assert same(got, want)
