"""No result of the dense flow (vs_flow.hip) or of the border fill (vs_fill.hip) may depend on memory the library never wrote.

The protocol of tests/test_uninitialised_memory_gpu.py -- VS_TEST_POISON_ALLOC=<byte> fills every fresh device allocation with that byte, the
same battery runs in one child process per byte, the digests of every status and output must be equal -- with the battery that module predates.
The flow keeps ten regions in one scratch block that is reused across layers, chunks and calls; bytes 255 and 0x7f read as NaN and 3.4e38 in a
float plane, so a flow that touched an unwritten float is not merely different, it is not finite: the battery asserts that as well."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
from video_stabilizer_amd import capi as G, synth
import _flow_cases as K
dig = hashlib.sha256()
def put(*xs):
    for x in xs:
        dig.update(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
def flow(f, a, b):
    fl = f.compute(a, b)
    assert np.isfinite(fl).all(), "a flow that is not finite"
    put(fl)
def jitter(f, clip):
    med, pm = f.jitter(clip)
    assert np.isfinite(med) and np.isfinite(pm).all(), "a pair median that is not finite"
    put(med, pm)
# (1) the hostile content classes, compute and jitter on one handle each
for name in K.CONTENT:
    a, b, kw, _ = K.content(name)
    f = G.Flow(G.flow_params(**kw))
    flow(f, a, b); jitter(f, np.stack([a, b, a]))
# (2) frames smaller than every halo, three parameter sets, layers that collapse to 1 x 1
for kw in K.PARAM_SETS[:3]:
    f = G.Flow(G.flow_params(levels=3, **kw))
    for w, h in K.TINY_SHAPES:
        a, b = K.small_pair(w, h, seed=w + 3 * h)
        flow(f, a, b); jitter(f, np.stack([a, b]))
# (3) a clip cut into two chunks (15 frames at 1920 x 1080), then small calls on the same handle: its scratch keeps the large call's data
t = K.u8(K.band_limited(1080, 1920, 5))
big = np.stack([np.roll(t, (3 * i %% 7 - 3, 5 * i %% 11 - 5), (0, 1)) for i in range(15)])
f = G.Flow()
jitter(f, big)
a, b = K.moving_pair(97, 61, seed=2)
flow(f, a, b); jitter(f, np.stack([a, b, a, b])); flow(f, *K.small_pair(5, 3, seed=1)); jitter(f, big[:2, :200, :300])
flow(f, big[0], big[1])
# (4) the border fill: short candidate lists, a list of one, an output that nothing covers
rng = np.random.default_rng(77)
w, h, n_src = 203, 149, 5
for dtype, maxv in ((np.uint8, 255), (np.uint16, 1023)):
    src = rng.integers(0, maxv + 1, (n_src, h, w, 3)).astype(dtype)
    cf = np.array([[0, 1, -1, -1], [1, -1, -1, -1], [2, 3, 4, 0], [3, 4, -1, 2]], np.int32)
    ct = [[G.Transform.of(rng.uniform(-0.02, 0.02), rng.uniform(-0.03, 0.03), rng.uniform(-25, 25), rng.uniform(-18, 18)) for _ in range(4)] for _ in range(4)]
    ct[3] = [G.Transform.of(0.0, 0.0, 5000.0 + 100 * c, -3000.0) for c in range(4)]          # output 3: no candidate covers anything
    for border in (G.BORDER_CONSTANT, G.BORDER_CLAMP):
        put(G.bgr_image_warp_fill_batch(src, cf, ct, border=border, max_value=maxv))
        put(G.bgr_image_warp_fill_batch(src, cf, ct, roi=(13, 9, 131, 77), border=border, max_value=maxv, dst_stride=3 * 131 + 2))
# (5) the stabilizer with the fill on over a clip with a scene cut, frame by frame and as a batch
clip = synth.make_clip(320, 240, 30, seed=5, channels=3)[0]
clip = np.concatenate([clip[:14], synth.make_clip(320, 240, 3, seed=77, channels=3)[0], clip[14:]])
kw = dict(device=0, lag=6, crop_pixels=8, border_fill=4)
s = G.Stabilizer(**kw)
for fr in clip:
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


@pytest.mark.parametrize("byte", [255, 0x7f, None], ids=["0xff", "0x7f", "unpoisoned"])
def test_flow_and_fill_do_not_depend_on_what_fresh_allocations_contain(gpu_vs, byte):
    # one child process per fill byte; every case compares with the zero-filled run (the first case pays for both)
    assert _digest(byte) == _digest(0)
