"""The fill's blend (vs_fill.hip: vs_k_bgr_channel_sums, vs_k_fill_gains, vs_k_bgr_warp_cv_fill_blend_c3) on inputs no moderate clip reaches: NaN /
singular / saturating maps (tests/_hostile_maps.py) as candidate 0 and as later candidates, maps that put cvRound and the 16-bit sampler on ties,
black frames (sums of 0), sum ratios far outside the gain's clamp, fresh allocations filled with a poison byte -- bit for bit against the rule's
reference (tests/_fill_blend_ref.py), every premise asserted on the CPU first.  All kernel-level calls work on device memory with guard bands on
the four sides of the destination windows and on both sides of the sums (tests/_fill_blend_direct.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _fill_blend_direct as D
import _fill_blend_ref as B
import _fill_ref as RF
import _hostile_maps as HM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(8, 255, np.uint8), (10, 1023, np.uint16), (16, 65535, np.uint16)]
IDENT = (0.0, 0.0, 0.0, 0.0)


def _ref(O, src, cf, maps, sums, feather, match, border, maxv, roi=None):
    with np.errstate(all="ignore"):
        return B.blend_batch(O, src, cf, [[O.Transform.of(*t) for t in row] for row in maps], sums, feather, match, border, maxv, roi)


@pytest.mark.parametrize("bits,maxv,dtype", KINDS[:2], ids=["8bit", "bgr10"])
def test_hostile_maps_as_candidate_0_and_as_later_candidates(gpu_vs, oracle, bits, maxv, dtype):
    """NaN, infinite, singular, near-singular, quarter-turn maps; translations beyond the 2^29 table-term guard, beyond cvRound's saturation and
    beyond everything; the near-singular transforms on which int64 and int32 coverage part (premise) -- each once as candidate 0 in front of two
    ordinary candidates and once as candidate 1 behind an ordinary candidate 0 that leaves a border and a band"""
    vs, O = gpu_vs, oracle
    w, h = 64, 48
    rng = np.random.default_rng(3 * bits)
    src = D.frames(rng, 4, w, h, dtype, maxv)
    sums = B.channel_sums(src)
    hostile = dict(HM.HOSTILE)
    hostile.update(HM.FILL_EXTREME)
    hostile["row0_trap"] = HM.row0_trap(vs, w, h)
    for n in HM.NEAR_SINGULAR:
        t = O.Transform.of(*hostile[n])
        assert not np.array_equal(RF.covered(O, t, w, h), RF.covered_int64(O, t, w, h)), n
    names = sorted(hostile)
    own = (0.02, -0.03, 7.0, -5.0)
    assert 0.3 < RF.covered(O, O.Transform.of(*own), w, h).mean() < 0.95
    maps = [[hostile[n], (0.01, 0.02, -3.0, 2.0), IDENT] for n in names] + [[own, hostile[n], (0.0, 0.0, 0.25, -0.25)] for n in names]
    cf = np.array([[i % 4, (i + 1) % 4, (i + 2) % 4] for i in range(len(maps))], np.int32)
    for feather, match, border in ((3, 1, vs.BORDER_CONSTANT), (6, 0, vs.BORDER_CLAMP), (0, 1, vs.BORDER_CLAMP)):
        want = _ref(O, src, cf, maps, sums, feather, match, border, maxv)
        got = D.dev_blend(vs, src, cf, maps, sums, feather, match, border=border, maxv=maxv)
        bad = [(names[i % len(names)], i // len(names)) for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (feather, match, bad)
    # one-row and one-column windows at frame row / column 0: a rectangle there has equal terms at both ends, only the deltas can be extreme
    for roi in ((0, 0, w, 1), (3, 0, 33, 1), (0, 0, 1, h)):
        want = _ref(O, src, cf, maps, sums, 4, 1, vs.BORDER_CONSTANT, maxv, roi)
        got = D.dev_blend(vs, src, cf, maps, sums, 4, 1, roi=roi, maxv=maxv)
        bad = [(names[i % len(names)], i // len(names)) for i in range(len(maps)) if not np.array_equal(got[i], want[i])]
        assert not bad, (roi, bad)


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10", "bgr16"])
def test_rint_ties(gpu_vs, oracle, bits, maxv, dtype):
    """translations of (n + 1/2) / 1024 put cvRound((M y + t) 1024) on a tie in every row (premise: the table terms in front of the rounding end
    in .5), half-pixel translations put the 16-bit sampler's rounding on ties wherever neighbouring samples differ by an odd amount (premise)"""
    vs, O = gpu_vs, oracle
    w, h = 67, 33
    rng = np.random.default_rng(bits + 9)
    src = D.frames(rng, 3, w, h, dtype, maxv)
    sums = B.channel_sums(src)
    table_ties = [(0.0, 0.0, 3.0 + 0.5 / 1024, -2.0 - 1.5 / 1024), (0.0, 0.0, -4.0 - 2.5 / 1024, 1.0 + 0.5 / 1024)]
    for t in table_ties:
        M = np.asarray(O.cv_inverse_matrix(O.Transform.of(*t), w, h), np.float64).reshape(6)
        assert (M[2] * 1024) % 1 == 0.5 and (M[5] * 1024) % 1 == 0.5, M
    half = [(0.0, 0.0, 2.5, -1.5), (0.0, 0.0, -3.5, 0.5)]
    a = src[1].astype(np.int64)
    assert ((a[:, 1:] + a[:, :-1]) % 2 == 1).mean() > 0.2             # sums of neighbours that are odd: (p + q) / 2 ends in .5
    maps = [[table_ties[0], half[0], table_ties[1]], [half[1], table_ties[1], half[0]], [(0.01, 0.0, 3.5, 2.5), half[0], half[1]]]
    cf = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0]], np.int32)
    for feather, match in ((0, 1), (2, 0), (5, 1)):
        for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
            want = _ref(O, src, cf, maps, sums, feather, match, border, maxv)
            got = D.dev_blend(vs, src, cf, maps, sums, feather, match, border=border, maxv=maxv)
            assert np.array_equal(got, want), (feather, match, border, int((got != want).sum()))


@pytest.mark.parametrize("bits,maxv,dtype", KINDS, ids=["8bit", "bgr10", "bgr16"])
def test_black_frames_and_extreme_sum_ratios(gpu_vs, oracle, bits, maxv, dtype):
    """a black output frame (S_k = 0), a black candidate (S_j = 0), one black channel: the gain is 32768 there (premise, on the device's own
    sums); then sums handed in by the caller at ratios far outside [1/2, 2], at the largest value the rule admits, and on the rounded division's
    tie: the gains clamp (premises) and a full-scale sample times 65536 saturates at max_value without wrapping"""
    vs, O = gpu_vs, oracle
    w, h = 70, 37
    rng = np.random.default_rng(bits + 21)
    src = D.frames(rng, 5, w, h, dtype, maxv)
    src[0] = 0                                                       # black
    src[1][..., 1] = 0                                               # one channel black
    src[4] = maxv                                                    # full scale
    fmt = {8: vs.FMT_BGR8, 10: vs.FMT_BGR10, 16: HM.FORMATS["bgr16"][0]}[bits]
    sums = D.dev_sums(vs, src, fmt)
    assert np.array_equal(sums, B.channel_sums(src))
    assert sums[0].tolist() == [0, 0, 0] and sums[1][1] == 0 and sums[1][0] > 0
    own = (0.02, -0.03, 6.0, -4.0)
    maps = [[own, (0.0, 0.01, 0.3, 0.6), IDENT]] * 4
    cf = np.array([[0, 2, 3], [2, 0, 3], [1, 2, 3], [3, 1, 4]], np.int32)
    assert B.gain_q15(sums[0][0], sums[2][0]) == 32768 and B.gain_q15(sums[2][0], sums[0][0]) == 32768 and B.gain_q15(sums[1][1], sums[2][1]) == 32768
    for feather in (0, 3):
        want = _ref(O, src, cf, maps, sums, feather, 1, vs.BORDER_CONSTANT, maxv)
        got = D.dev_blend(vs, src, cf, maps, sums, feather, 1, maxv=maxv)
        assert np.array_equal(got, want), (feather, int((got != want).sum()))
    # black frames against each other: with a zero sum on either side the match changes nothing
    two, two_maps = cf[:2, :2], [row[:2] for row in maps[:2]]         # (black output with a candidate, an output with a black candidate)
    assert np.array_equal(D.dev_blend(vs, src, two, two_maps, sums, 3, 1, maxv=maxv), D.dev_blend(vs, src, two, two_maps, None, 3, 0, maxv=maxv))
    big = 65535 * 32767 * 32767
    fake = np.array([[1, big, 40001], [big, 1, 65536], [big, big, 39999], [3, 1000, big // 2 + 1], [1, 1, 1]], np.uint64)
    assert [B.gain_q15(fake[0][c], fake[1][c]) for c in range(3)] == [16384, 65536, 20001]
    assert [B.gain_q15(fake[2][c], fake[1][c]) for c in range(3)] == [32768, 65536, 19999 + 1]
    assert B.gain_q15(fake[0][0], fake[4][0]) == 32768 and B.gain_q15(fake[1][0], fake[4][0]) == 65536
    cf = np.array([[0, 1, 2], [2, 1, 0], [1, 4, 3], [3, 0, 4], [0, 4, 1]], np.int32)
    maps = [[own, (0.0, 0.01, 0.3, 0.6), IDENT]] * 5
    for feather in (0, 4):
        want = _ref(O, src, cf, maps, fake, feather, 1, vs.BORDER_CLAMP, maxv)
        got = D.dev_blend(vs, src, cf, maps, fake, feather, 1, border=vs.BORDER_CLAMP, maxv=maxv)
        assert np.array_equal(got, want), (feather, int((got != want).sum()))
    assert want.max() == maxv                                        # the full-scale frame at gain 65536: saturated, not wrapped


def test_samples_above_max_value(gpu_vs, oracle):
    """a bgr10 container that holds 65535 and 1024 at scattered pixels, max_value 1023: the sampler's saturation and the clamp behind the gain are
    live (premise: the result under max_value 65535 differs); the sums count the raw samples"""
    vs, O = gpu_vs, oracle
    w, h = 131, 77
    rng = np.random.default_rng(10)
    src = D.frames(rng, 3, w, h, np.uint16, 1023)
    src[1][rng.random((h, w)) < 0.1] = 65535
    src[2][rng.random((h, w, 3)) < 0.1] = 1024
    sums = D.dev_sums(vs, src, vs.FMT_BGR10)
    assert np.array_equal(sums, B.channel_sums(src)) and sums[1].min() > 1023 * w * h // 2
    maps = [[(0.03, -0.04, 11.0, -8.0), (0.0, 0.01, 0.3, 0.6), (0.01, 0.0, -0.4, 0.2)], [(-0.02, 0.05, -9.0, 6.0), (0.0, 0.0, 0.5, 0.5), IDENT]]
    cf = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    want = _ref(O, src, cf, maps, sums, 3, 1, vs.BORDER_CONSTANT, 1023)
    loose = _ref(O, src, cf, maps, sums, 3, 1, vs.BORDER_CONSTANT, 65535)
    assert (loose > 1023).any() and want.max() == 1023 and not np.array_equal(want, loose)
    for border in (vs.BORDER_CONSTANT, vs.BORDER_CLAMP):
        got = D.dev_blend(vs, src, cf, maps, sums, 3, 1, border=border, maxv=1023)
        assert np.array_equal(got, _ref(O, src, cf, maps, sums, 3, 1, border, 1023))


K_SLOTS = 1 << 15                                                    # the parameter ring's slots


def test_the_second_group_of_a_long_call(gpu_vs, oracle):
    """the candidates' entries travel in groups of (kSlots / 2 / 4) / n_cand output frames -- 256 at 16 candidates -- and the gain kernel rewrites
    them in place: n_out = group + 3 crosses the seam (the second group's entries, sums pointers and destination offsets)"""
    vs, O = gpu_vs, oracle
    n_cand = 16
    group = min(K_SLOTS // 2 // 3, (K_SLOTS // 2 // 4) // n_cand)
    assert group == 256
    n_out = group + 3
    w, h, n_src = 12, 9, 6
    rng = np.random.default_rng(n_cand)
    src = D.frames(rng, n_src, w, h, np.uint8, 255)
    sums = B.channel_sums(src)
    cf = rng.integers(0, n_src, (n_out, n_cand)).astype(np.int32)
    maps = [[(rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1), rng.uniform(-2, 2), rng.uniform(-2, 2)) for _ in range(n_cand)] for _ in range(n_out)]
    want = _ref(O, src, cf, maps, sums, 1, 1, vs.BORDER_CONSTANT, 255)
    plain = RF.fill_batch(O, src, cf, [[O.Transform.of(*t) for t in row] for row in maps], vs.BORDER_CONSTANT, 255)
    assert all((plain[o] != want[o]).any() for o in range(group - 2, n_out))
    got = D.dev_blend(vs, src, cf, maps, sums, 1, 1, maxv=255)
    bad = [o for o in range(n_out) if not np.array_equal(got[o], want[o])]
    assert not bad, (bad[:8], len(bad))


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
from video_stabilizer_amd import capi as G, synth
dig = hashlib.sha256()
def put(*xs):
    for x in xs:
        dig.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
rng = np.random.default_rng(78)
w, h, n_src = 203, 149, 5
for dtype, maxv, fmt in ((np.uint8, 255, G.FMT_BGR8), (np.uint16, 1023, G.FMT_BGR10)):
    src = rng.integers(0, maxv + 1, (n_src, h, w, 3)).astype(dtype)
    sums = G.channel_sums_batch(src, fmt=fmt)
    put(sums, G.channel_sums_batch(src, fmt=fmt, src_stride=3 * w + 5))
    cf = np.array([[4, 0, -1, -1], [1, -1, -1, -1], [2, 3, 4, 0], [3, 4, -1, 2], [0, 1, 2, 3]], np.int32)
    ct = [[G.Transform.of(rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03), rng.uniform(-15, 15), rng.uniform(-15, 15)) for _ in range(4)] for _ in range(5)]
    ct[0][0] = G.Transform.of(0.0, 0.0, 5000.0, -3000.0)
    for feather, match in ((0, 1), (4, 0), (6, 1)):
        put(G.bgr_image_warp_fill_blend_batch(src, cf, ct, sums, feather, match, max_value=maxv))
        put(G.bgr_image_warp_fill_blend_batch(src, cf, ct, sums, feather, match, max_value=maxv, src_stride=3 * w + 7, dst_stride=3 * w + 5))
clip = synth.make_clip(320, 240, 20, seed=5, channels=3)[0]
clip = np.concatenate([clip[:9], synth.make_clip(320, 240, 3, seed=77, channels=3)[0], clip[9:]])
clip = (clip * (0.9 + 0.02 * (np.arange(len(clip)) %% 7))[:, None, None, None]).astype(np.uint8)
for kw in (dict(fill_blend=(4, 1)), dict(fill_blend=(0, 1), deblur=3, denoise=2), dict(fill_blend=(5, 0))):
    kw = dict(dict(device=0, lag=5, crop_pixels=0, border_fill=4), **kw)
    s = G.Stabilizer(**kw)
    for i, fr in enumerate(clip):
        if i == 7 and kw["fill_blend"] == (5, 0):
            s.set_fill_blend(2, 1)                                   # switched on mid-clip: the queued frames are summed into a fresh block
        o = s.process(fr)
        put(o is None)
        if o is not None:
            put(o)
    out, has = G.Stabilizer(**kw).process_batch(clip)
    put(has, out[np.array(has, bool)])
print("DIGEST", dig.hexdigest())
"""

_digests = {}


def _digest(byte):
    if byte not in _digests:
        env = dict(os.environ)
        env.pop("VS_TEST_POISON_ALLOC", None)
        if byte is not None:
            env["VS_TEST_POISON_ALLOC"] = str(byte)
            env["VS_TEST_HOOKS"] = "1"
        out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        _digests[byte] = [line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1]
    return _digests[byte]


@pytest.mark.parametrize("byte", [255, None], ids=["0xff", "unpoisoned"])
def test_blend_does_not_depend_on_what_fresh_allocations_contain(gpu_vs, byte):
    # one child process per fill byte; every case compares with the zero-filled run (the first case pays for both)
    assert _digest(byte) == _digest(0)
