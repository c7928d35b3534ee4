"""The resize pass (vs_resize.hip) on hostile input: samples above the format's maximum, checkerboards of 0 and the maximum at every phase --
the 16-bit ones drive the 64-bit sum to 4096 * 4096 * 65535 --, frames inside poison on all four sides and destinations inside guard bands
(tests/test_resize_gpu.py: dev_resize), poisoned allocations, every allocation of a call failed once.  Bit for bit against the rule's
restatement (tests/_resize_ref.py); every case asserts its premise on the restatement before it looks at the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _resize_ref as R
from _stab_routes import walk
from test_resize_gpu import FORMATS, dev_resize

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(70, 37, 23, 11, R.AREA), (70, 37, 35, 19, R.LINEAR), (33, 21, 70, 37, R.LINEAR), (64, 64, 8, 8, R.AREA), (45, 30, 44, 31, R.LINEAR)]


@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum_count_as_the_maximum(gpu_vs, fmt):
    """10- and 12-bit containers that hold 65535 and max_value + 1 at scattered samples.  Premises: the cut is live (the result under
    max_value 65535 differs) and no output exceeds the maximum"""
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    rng = np.random.default_rng(bits)
    for sw, sh, dw, dh, filt in SHAPES:
        src = rng.integers(0, maxv + 1, (2, sh, sw, 3)).astype(dtype)
        for f in src:
            f[rng.random((sh, sw)) < 0.08] = 65535
            f[rng.random((sh, sw, 3)) < 0.05] = maxv + 1
        want = R.resize(src, dw, dh, filt, maxv)
        assert not np.array_equal(want, R.resize(src, dw, dh, filt, 65535)) and want.max() <= maxv
        got = dev_resize(gpu_vs, src, dw, dh, code, filt, src_guard=65535)
        assert np.array_equal(got, want), (sw, sh, dw, dh, filt, int((got != want).sum()))


@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_checkerboards_of_zero_and_the_maximum_at_every_phase(gpu_vs, fmt):
    """cells of 1, 2 and 3 pixels, shifted through every phase of the destination grid, and the all-maximum frame.  Premises: the restatement
    keeps the extremes (an all-maximum frame stays all-maximum: V = 4096 * 4096 * max_value; some shape keeps a 0), the boards give values
    strictly between"""
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    zero_kept = False
    for sw, sh, dw, dh, filt in SHAPES:
        boards = [np.full((sh, sw, 3), maxv, dtype)]
        yy, xx = np.mgrid[0:sh, 0:sw]
        for cell in (1, 2, 3):
            for phase in range(2 * cell):
                b = (((xx + phase) // cell + (yy + phase // 2) // cell) & 1).astype(dtype) * maxv
                boards.append(np.repeat(b[..., None], 3, axis=2))
        src = np.stack(boards)
        want = R.resize(src, dw, dh, filt, maxv)
        assert (want[0] == maxv).all() and ((want[1:] > 0) & (want[1:] < maxv)).any()
        zero_kept = zero_kept or bool((want == 0).any())
        got = dev_resize(gpu_vs, src, dw, dh, code, filt, src_guard=maxv // 3)
        assert np.array_equal(got, want), (sw, sh, dw, dh, filt, int((got != want).sum()))
    assert zero_kept


CHILD = r"""
import hashlib, sys
sys.path.insert(0, %(root)r)
import numpy as np
from video_stabilizer_amd import capi as G, synth
dig = hashlib.sha256()
rng = np.random.default_rng(5)
for dtype, maxv, fmt in ((np.uint8, 255, G.FMT_BGR8), (np.uint16, 1023, G.FMT_BGR10)):
    for sw, sh, dw, dh, filt in ((261, 33, 130, 17, G.RESIZE_AREA), (129, 65, 200, 99, G.RESIZE_LINEAR), (2, 1, 1, 1, G.RESIZE_AREA), (40, 700, 23, 19, G.RESIZE_LINEAR)):
        img = rng.integers(0, maxv + 1, (3, sh, sw, 3)).astype(dtype)
        for kw in (dict(), dict(src_stride=3 * sw + 7, dst_stride=3 * dw + 5)):
            dig.update(G.resize_batch(img, dw, dh, filt, fmt=fmt, **kw).tobytes())
clip = np.maximum(synth.make_clip(96, 64, 14, seed=5, channels=3)[0], 1)
for size in ((-1, -1), (50, 30)):
    kw = dict(device=0, lag=4, crop_pixels=8, output_size=size, sharpen=True, pyramid_min_width=10, pyramid_min_height=10)
    s = G.Stabilizer(**kw)
    for fr in clip:
        o = s.process(fr)
        dig.update(b"-" if o is None else o.tobytes())
    out, has = G.Stabilizer(**kw).process_batch(clip)
    dig.update(repr(has).encode() + out[np.array(has, bool)].tobytes())
print("DIGEST", dig.hexdigest())
"""


def test_the_resize_does_not_depend_on_what_fresh_allocations_contain(gpu_vs):
    """one child process per fill byte of every fresh device allocation (VS_TEST_POISON_ALLOC): the kernel-level call and the engine with the
    output size set give the same bytes"""
    digests = []
    for byte in (255, 0):
        env = dict(os.environ, VS_TEST_POISON_ALLOC=str(byte), VS_TEST_HOOKS="1")
        out = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        digests.append([line for line in out.stdout.splitlines() if line.startswith("DIGEST")][-1].split()[1])
    assert digests[0] == digests[1]


@pytest.mark.parametrize("throwing", [False, True])
def test_resize_batch_survives_every_allocation_failure(gpu_vs, throwing):
    """the kernel-level call on host memory (frames and output are staged): every allocation failed once"""
    vs = gpu_vs
    rng = np.random.default_rng(9)
    # (a size no other test stages: the walk starts from an empty spot of the staging pool or from a warm one, and ends either way)
    src = rng.integers(0, 256, (3, 39, 213, 3)).astype(np.uint8)
    want = R.resize(src, 101, 17, R.AREA, 255)

    def call(_):
        return vs.resize_batch(src, 101, 17, vs.RESIZE_AREA).tobytes()
    assert call(None) == want.tobytes()
    walk(vs, lambda: None, call, 0, throwing)
