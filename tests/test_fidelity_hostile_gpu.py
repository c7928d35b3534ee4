"""The fidelity statistics kernel (vs_fidelity.hip) on hostile input: samples above the format's maximum on either side, all-0 against all-maximum at
16 bits (one squared difference overflows a 32-bit accumulator), the checkerboard against its inverse (a negative ssim_sum), repeats of one call --
bit for bit against the rule's restatement (tests/_fidelity_ref.py).  Every case asserts its premise on the restatement before it looks at the GPU.

All calls work on DEVICE memory: the images lie inside a band of poison on all four sides (a sample read outside an image would show in the sums),
the statistics between guard words, in a buffer filled with poison first -- so the zeroes under the sums are the launcher's."""
import numpy as np
import pytest

import _fidelity_ref as R
from _diff import same
from test_fidelity_gpu import BAND, FORMATS, STRIP

pytestmark = pytest.mark.gpu

G = 3
GUARD64 = 0x5A5A5A5A5A5A5A5A


def _dev_stats(vs, a, b, pairs, fmt, poison=None, repeats=1):
    """vs_bgr_fidelity_batch on device memory -> (n_pairs, 6) uint64.  Image i of a batch lies at rows G .. G + h, columns G .. G + w of a
    (h + 2 G) x (w + 2 G) picture of `poison`; the statistics lie between G guard words a side, over poison"""
    import torch
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    _, h, w, _ = a.shape
    esz = a.dtype.itemsize
    poison = (0x5A if esz == 1 else 0x5A5A) if poison is None else poison
    ss = 3 * (w + 2 * G)
    fs = (h + 2 * G) * ss

    def upload(src):
        host = np.full((src.shape[0], h + 2 * G, ss), poison, src.dtype)
        host[:, G:G + h, 3 * G:3 * G + 3 * w] = src.reshape(src.shape[0], h, 3 * w)
        return host, torch.from_numpy(host.view(np.int16) if esz == 2 else host).cuda()
    ha, da = upload(a)
    hb, db = upload(b)
    n_pairs = len(pairs)
    org = (G * ss + 3 * G) * esz
    outs = []
    for _ in range(repeats):
        dstats = torch.from_numpy(np.full(6 * n_pairs + 2 * G, GUARD64, np.uint64).view(np.int64)).cuda()
        torch.cuda.synchronize()
        vs.fidelity_stats_batch_device(da.data_ptr() + org, fs, a.shape[0], ss, db.data_ptr() + org, fs, b.shape[0], ss, w, h, fmt, pairs,
                                       dstats.data_ptr() + 8 * G)
        torch.cuda.synchronize()
        st = dstats.cpu().numpy().view(np.uint64)
        assert (st[:G] == GUARD64).all() and (st[-G:] == GUARD64).all(), "words round the statistics were written"
        outs.append(st[G:-G].reshape(n_pairs, 6).copy())
    assert same(da.cpu().numpy().view(a.dtype), ha) and np.array_equal(db.cpu().numpy().view(b.dtype), hb), "the images were written"
    return outs[0] if repeats == 1 else outs


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples, on side a alone, on side b alone and on both: they count
    as the maximum.  Premise: the clamp is live -- on the raw samples every SSE word differs"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for w, h in ((131, 37), (STRIP + 3, 20)):
        a = rng.integers(0, maxv + 1, (4, h, w, 3)).astype(dtype)
        b = rng.integers(0, maxv + 1, (4, h, w, 3)).astype(dtype)
        for f in (a[2], a[3], b[0], b[1]):
            f[rng.random((h, w)) < 0.08] = 65535
            f[rng.random((h, w, 3)) < 0.05] = maxv + 1
        pairs = [(2, 2), (0, 0), (3, 1), (1, 3)]                         # above the maximum on side a, on side b, on both, on neither
        want = R.stats_batch(a, b, pairs, bits)
        raw = [int(((a[i].astype(np.int64) - b[j].astype(np.int64))[..., c] ** 2).sum()) for i, j in pairs[:3] for c in range(3)]
        assert all(r != int(v) for r, v in zip(raw, want[:3, :3].ravel()))
        assert same(_dev_stats(vs, a, b, pairs, code), want), (w, h)


def test_all_zero_against_all_maximum_at_16_bits(gpu_vs):
    """every pixel adds 65535^2 = 4 294 836 225 to each channel's word: one already exceeds 2^31, two exceed 2^32.  Two strips by two bands"""
    vs = gpu_vs
    code, dtype, bits = FORMATS["bgr16"]
    w, h = STRIP + 5, BAND + 6
    a = np.stack([np.zeros((h, w, 3), dtype), np.full((h, w, 3), 65535, dtype)])
    pairs = [(0, 1), (1, 0), (1, 1)]
    want = R.stats_batch(a, a, pairs, bits)
    nw = R.n_windows(w, h)[0] * R.n_windows(w, h)[1]
    assert want.tolist() == [[65535 * 65535 * w * h] * 3 + [65025 * w * h, nw, 7 * nw]] * 2 + [[0, 0, 0, 0, nw, 65536 * nw]]
    assert 65535 * 65535 > 1 << 31 and int(want[0, 0]) > 1 << 46
    assert same(_dev_stats(vs, a, a, pairs, code, poison=0x1234), want)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_all_zero_against_all_maximum(gpu_vs, fmt):
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = 21, 13
    top = 65535 if bits > 8 else 255
    a = np.stack([np.zeros((h, w, 3), dtype), np.full((h, w, 3), top, dtype), np.full((h, w, 3), maxv, dtype)])
    want = R.stats_batch(a, a, [(0, 1), (2, 0), (1, 2)], bits)
    assert want.tolist() == [[maxv * maxv * w * h] * 3 + [65025 * w * h, 8, 7 * 8]] * 2 + [[0, 0, 0, 0, 8, 65536 * 8]]
    assert same(_dev_stats(vs, a, a, [(0, 1), (2, 0), (1, 2)], code, poison=0), want)


def test_the_checkerboard_gives_a_negative_ssim_sum(gpu_vs):
    vs = gpu_vs
    w, h = STRIP + 9, BAND + 9
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.repeat(((((xx + yy) & 1) * 255).astype(np.uint8))[:, :, None], 3, axis=2)
    a = np.stack([c, 255 - c])
    pairs = [(0, 1), (1, 0), (0, 0)]
    want = R.stats_batch(a, a, pairs, 8)
    nw = R.n_windows(w, h)[0] * R.n_windows(w, h)[1]
    assert R.ssim_sum_signed(want[0, 5]) == -65300 * nw and int(want[0, 5]) > 1 << 63 and nw > 1000
    got = _dev_stats(vs, a, a, pairs, 1)
    assert same(got, want)
    assert vs.fidelity_scores(got, w, h)[:, 5].tolist() == [-65300.0 / 65536.0, -65300.0 / 65536.0, 1.0]


@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_three_repeats_of_one_call_are_identical(gpu_vs, fmt):
    """the partial sums of the waves meet in atomics, in any order: integer sums do not care"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    rng = np.random.default_rng(40 + bits)
    w, h = 2 * STRIP + 30, 2 * BAND + 11
    a = rng.integers(0, 1 << bits, (3, h, w, 3)).astype(dtype)
    b = np.clip(a.astype(np.int64) + rng.integers(-(1 << (bits - 4)), 1 << (bits - 4), a.shape), 0, (1 << bits) - 1).astype(dtype)
    pairs = [(0, 0), (1, 2), (2, 1), (1, 1)]
    want = R.stats_batch(a, b, pairs, bits)
    outs = _dev_stats(vs, a, b, pairs, code, repeats=3)
    assert all(np.array_equal(o, want) for o in outs)
