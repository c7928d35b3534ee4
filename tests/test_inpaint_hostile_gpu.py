"""The inpaint's two kernel-level calls (vs_inpaint.hip) where the first tests never went.  Coverage index: rotations that put the coverage
boundary diagonally across blocks and strips, windows of 1 .. 257 pixels at odd offsets, NaN / singular / near-singular / saturating maps as
candidate 0 and behind it, frames in which nothing can be covered, the index value 16, the C ABI's candidate-group seam.  Push-pull: the
tail's edges (exactly 4096 texels from the image and from the pyramid, one row over, the 8191-texel LDS maximum of 1 x 4096), inputs on which
each of the rule's two roundings decides, mask bytes >= 0x80, samples above the format's maximum, open counts of 0, 1, w h - 1 and w h in one
batch, and the 65535-frame line of gridDim.y.  Bytes for bytes against the rule (tests/_inpaint_ref.py on tests/_fill_ref.py); inputs,
premises and the device-memory drivers (guard band on four sides, both pitch alignments): tests/_inpaint_cases.py.  Every premise is asserted
on the CPU references before a kernel runs.  The stabilizer's scratch groups run in child processes (VS_TEST_INPAINT_SCRATCH_BYTES)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _inpaint_cases as IC
import _inpaint_ref as R
import test_inpaint_gpu as TI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the coverage index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cand", [5, 16])
@pytest.mark.parametrize("w,h", [(300, 270), (520, 70)], ids=["300x270", "520x70"])
def test_index_under_large_rotations(gpu_vs, oracle, w, h, n_cand):
    """2 x 2 and 3 x 1 blocks under rotations up to +-0.5 rad; the full frame, then windows whose sides are 1, 63, 65, 256 and 257 at
    offsets that are no multiples of 64: each equals the crop of the full index"""
    cf, maps, full = IC.rotation_case(oracle, w, h, n_cand)
    rois = IC.rotation_rois(w, h)
    for roi in [None] + rois:
        bad = IC.check_index(gpu_vs, w, h, cf, maps, full, roi)
        assert not bad, (roi, bad)


def test_index_under_hostile_maps(gpu_vs, oracle):
    w, h = 64, 48
    cf, maps, full, label = IC.hostile_case(oracle, w, h)
    for roi in (None, (0, 0, w, 1), (3, 0, 33, 1), (0, 0, 1, h)):
        bad = IC.check_index(gpu_vs, w, h, cf, maps, full, roi)
        assert not bad, (roi, [label[k] for k in bad])


def test_index_of_frames_in_which_nothing_or_one_position_can_be_covered(gpu_vs, oracle):
    for w, h, cf, maps, full in IC.nothing_covered_cases(oracle):
        assert not IC.check_index(gpu_vs, w, h, cf, maps, full), (w, h)


def test_index_value_16_and_all_ones_with_sixteen_candidates(gpu_vs, oracle):
    w, h = 300, 270
    for cf, maps, full in IC.sixteen_case(oracle, w, h):
        for roi in (None, (21, 17, 257, 129)):
            assert not IC.check_index(gpu_vs, w, h, cf, maps, full, roi), (roi, sorted(np.unique(full)))


@pytest.mark.parametrize("n_cand,extra", [(16, 3), (1, 1)])
def test_index_across_the_candidate_group_seam(gpu_vs, oracle, n_cand, extra):
    w, h = 12, 9
    group, cf, maps, full = IC.seam_case(oracle, n_cand, extra, w, h)
    assert len(cf) == group + extra == {16: 259, 1: 4097}[n_cand]
    bad = IC.check_index(gpu_vs, w, h, cf, maps, full)
    assert not bad, (bad[:8], len(bad))


# ---- the push-pull -------------------------------------------------------------------------------------------------------------------------------
# 64 x 64: exactly kTailTexels from the image; 65 x 64: one texel row over, the tail starts at level 1; 128 x 128: exactly 4096 texels from
# the pyramid; 127 x 129: 64 x 65 = 4160 at level 1, one row over again; 1 x 4096 / 4096 x 1: 4096 + 2048 + ... + 1 = 8191 texels in the tail's
# LDS, the most any shape asks for; 1 x 4097 / 4097 x 1: the tail starts at level 1 with 2049 texels; 2 x 2048: the levels quarter once, then halve
TAIL_EDGES = [(64, 64), (65, 64), (128, 128), (127, 129), (1, 4096), (4096, 1), (1, 4097), (4097, 1), (2, 2048)]


@pytest.mark.parametrize("fmt", ["u8", "bgr16"])
@pytest.mark.parametrize("w,h", TAIL_EDGES, ids=["%dx%d" % s for s in TAIL_EDGES])
def test_tail_edges(gpu_vs, w, h, fmt):
    dtype, maxv = IC.FORMATS[fmt]
    rng = np.random.default_rng(w * 31 + h + maxv)
    masks = np.concatenate([TI._masks(rng, w, h), IC.corner_and_single_masks(w, h)])
    imgs = TI._content(rng, len(masks), w, h, dtype, maxv)
    opens = (masks == 0).sum((1, 2))
    assert {1, w * h - 1} <= set(opens.tolist()) and (opens[-3:] == 1).all() and masks[-3, 0, 0] == 0 and masks[-2, -1, -1] == 0
    bad = IC.check_inpaint(gpu_vs, imgs, masks, fmt)
    assert not bad, bad


@pytest.mark.parametrize("fmt", ["u8", "bgr16"])
@pytest.mark.parametrize("w,h", [(64, 4097), (4097, 64), (257, 5), (513, 3)], ids=["64x4097", "4097x64", "257x5", "513x3"])
def test_one_kept_and_one_open_pixel_at_the_corners(gpu_vs, w, h, fmt):
    """the deepest pyramids with one kept pixel in a corner (every other texel of every level comes from it); one open pixel in the last
    column of windows with w % 256 == 1 (the open count's second column pass)"""
    dtype, maxv = IC.FORMATS[fmt]
    rng = np.random.default_rng(w + h)
    masks = IC.corner_and_single_masks(w, h)
    imgs = TI._content(rng, len(masks), w, h, dtype, maxv)
    assert w % 256 == 1 or h % 256 == 1
    bad = IC.check_inpaint(gpu_vs, imgs, masks, fmt)
    assert not bad, bad


@pytest.mark.parametrize("fmt", ["u8", "bgr10", "bgr16"])
@pytest.mark.parametrize("w,h", [(63, 65), (300, 270)], ids=["63x65", "300x270"])
def test_inputs_on_which_the_roundings_decide(gpu_vs, w, h, fmt):
    for high in (0, 1):
        for open_share in (0.5, 0.9):
            img, mask, want = IC.rounding_case(w, h, fmt, high, open_share)
            assert not IC.check_inpaint(gpu_vs, img, mask, fmt, want), (high, open_share)


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
@pytest.mark.parametrize("w,h", [(131, 77), (300, 270)], ids=["131x77", "300x270"])
def test_mask_bytes_above_0x7f_and_samples_above_the_formats_maximum(gpu_vs, w, h, fmt):
    """the rule never clamps: max_value does not come into it"""
    img, mask, want = IC.out_of_range_case(w, h, fmt)
    bad = IC.check_inpaint(gpu_vs, img, mask, fmt, want)
    assert not bad, bad
    assert not IC.check_inpaint(gpu_vs, img, mask, fmt, want, host=True)


@pytest.mark.parametrize("fmt", ["u8", "bgr16"])
@pytest.mark.parametrize("w,h", [(300, 270), (60, 50)], ids=["300x270", "60x50"])
def test_idle_and_busy_frames_in_one_batch(gpu_vs, w, h, fmt):
    """open counts 0, w h, 1 and w h - 1 between busy frames, with the pyramid (300 x 270) and tail only (60 x 50); frame strides larger than a
    frame: idle frames and guards come back untouched (IC.dev_inpaint, IC.check_inpaint)"""
    imgs, masks, want = IC.idle_and_busy_batch(w, h, fmt)
    bad = IC.check_inpaint(gpu_vs, imgs, masks, fmt, want)
    assert not bad, bad


N_LINE = 65537                                                       # gridDim.y takes 65535 frames: two in the second launch group


def test_the_65535_frame_line_tail_only(gpu_vs):
    """65537 frames of 2 x 2 in host memory (the tail alone; the open count's and the inpaint's second launch groups).  The rule on 2 x 2
    windows is the rounded mean of the kept pixels (IC.inpaint_2x2; premise: it is the reference on every mask pattern)"""
    vs = gpu_vs
    rng = np.random.default_rng(65537)
    imgs = rng.integers(0, 256, (N_LINE, 2, 2, 3)).astype(np.uint8)
    masks = (rng.integers(0, 2, (N_LINE, 2, 2)) * rng.integers(1, 256, (N_LINE, 2, 2))).astype(np.uint8)
    masks[-4:] = [[[0, 5], [0, 0]], [[1, 0], [0, 0x80]], [[0, 0], [0, 0]], [[0xFF, 0], [7, 9]]]
    want = IC.inpaint_2x2(imgs, masks)
    probe = list(range(200)) + list(range(N_LINE - 6, N_LINE))
    assert len({(masks[k] != 0).tobytes() for k in probe}) == 16
    assert all(np.array_equal(want[k], R.inpaint(imgs[k], masks[k])) for k in probe)
    assert all(not np.array_equal(want[k], imgs[k]) for k in (N_LINE - 4, N_LINE - 3, N_LINE - 1))
    got = vs.bgr_inpaint_batch(imgs, masks)
    bad = np.flatnonzero((got != want).any((1, 2, 3)))
    assert bad.size == 0, (bad[:8], bad.size)


def test_the_65535_frame_line_with_a_pyramid(gpu_vs):
    """65537 frames of 65 x 64 (8 bits) in device memory: the tail starts at level 1, so the pyramid's frame offset crosses the line as
    well.  Image and mask are made on the device; frames 0 and 65533 .. 65536 are downloaded and compared with the rule (premise: each has
    open and kept pixels); property (a), kept pixels bit for bit, over the whole batch on the device"""
    import torch
    vs = gpu_vs
    w, h = 65, 64
    gen = torch.Generator(device="cuda").manual_seed(5)
    img = torch.randint(0, 256, (N_LINE, h, w, 3), dtype=torch.uint8, device="cuda", generator=gen)
    mask = torch.randint(0, 2, (N_LINE, h, w), dtype=torch.uint8, device="cuda", generator=gen) * 0x81
    before = img.clone()
    probe = [0, N_LINE - 4, N_LINE - 3, N_LINE - 2, N_LINE - 1]
    src = {k: (before[k].cpu().numpy(), mask[k].cpu().numpy()) for k in probe}
    assert all(0 < (m == 0).sum() < w * h for _, m in src.values())
    want = {k: R.inpaint(*src[k]) for k in probe}
    assert all(not np.array_equal(want[k], src[k][0]) for k in probe)
    torch.cuda.synchronize()
    vs.bgr_inpaint_batch_device(img.data_ptr(), h * w * 3, N_LINE, w, h, w * 3, vs.FMT_BGR8, mask.data_ptr(), h * w, w)
    torch.cuda.synchronize()
    for k in probe:
        assert np.array_equal(img[k].cpu().numpy(), want[k]), k
    keep = mask != 0
    assert not bool((((img != before).any(-1)) & keep).any())        # (a)
    changed = ((img != before).any(-1) & ~keep).reshape(N_LINE, -1).any(1)
    assert bool(changed.all())                                       # every frame was worked on (noise: some open pixel differs from its estimate)


# ---- the stabilizer's scratch groups -------------------------------------------------------------------------------------------------------------
CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, %(root)r)
import numpy as np
from video_stabilizer_amd import capi as G, synth
def clip(n, seed):
    return np.maximum(synth.make_clip(160, 128, n, seed=seed, channels=3)[0], 1)
a = clip(30, 5)
frames = np.concatenate([a[:14], clip(3, 77), a[14:]])                # 33 frames with a scene cut: the candidate lists end early there
def run(**kw):
    kw = dict(dict(device=0, lag=6, crop_pixels=0, border_fill=3), **kw)
    dig = hashlib.sha256()
    s = G.Stabilizer(**kw)
    for fr in frames:
        o = s.process(fr)
        dig.update(b"-" if o is None else np.ascontiguousarray(o).tobytes())
    out, has = G.Stabilizer(**kw).process_batch(frames)
    dig.update(repr(list(has)).encode() + np.ascontiguousarray(out[np.array(has, bool)]).tobytes())
    return dig.hexdigest()
on = run(inpaint=1)
if "VS_TEST_INPAINT_SCRATCH_BYTES" not in os.environ:
    assert on != run(inpaint=0), "the inpaint changed nothing on this clip"
print("DIGEST", on)
"""


def _child(budget):
    env = dict(os.environ, VS_TEST_HOOKS="1")
    env.pop("VS_TEST_INPAINT_SCRATCH_BYTES", None)
    if budget is not None:
        env["VS_TEST_INPAINT_SCRATCH_BYTES"] = str(budget)
    out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1]


def _pyramid_bytes(w, h, esz=1):
    """the pyramid's bytes per frame as Chunk::inpaint_run counts them: the levels 1 .. tail (the first of at most 4096 texels) of four
    container-sized elements, rounded up to 16 bytes"""
    texels = 0
    while w * h > 4096:
        w, h = (w + 1) >> 1, (h + 1) >> 1
        texels += w * h
    return (texels * 4 * esz + 15) & ~15


def test_the_stabilizers_scratch_groups_give_the_same_frames(gpu_vs):
    """inpaint_run splits a run where its scratch would pass the budget, offsets candidates and destination by the group's first frame and
    reuses counts, index and pyramid.  The 33-frame cut clip at 160 x 128, crop 0, fill 3, frame by frame and through process_batch, with a
    budget of one byte (one frame per group), with one that gives groups of three, and with the built-in one: the same bytes.  (A child
    process each: VS_TEST_HOOKS is read once per process.  Premise, in the child that runs without the hook: inpaint on differs from off.)"""
    w, h = 160, 128
    per_frame = w * h + _pyramid_bytes(w, h) + 4                   # index (rows of 160 bytes: dword-padded as they are), pyramid, count
    three = 3 * per_frame + per_frame // 2
    assert three // per_frame == 3
    plain = _child(None)
    assert _child(1) == plain
    assert _child(three) == plain

