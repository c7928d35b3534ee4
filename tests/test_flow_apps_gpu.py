"""-m gpu: the harness programs' --score flow (the reference's own dense-flow jitter score, this build's Farneback) and the
unchanged default (--score similarity)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_apps_gpu import BIN, ROOT, run  # noqa: E402

pytestmark = pytest.mark.gpu
W, H, N = 320, 240, 24


@pytest.fixture(scope="module")
def raw_clip(gpu_vs, tmp_path_factory):
    from video_stabilizer_amd import synth
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    d = tmp_path_factory.mktemp("flow_recordings")
    frames, _ = synth.make_clip(W, H, N, seed=78, channels=3)
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    return frames, raw


def test_eval_jitter_flow_prints_flow_jitter(gpu_vs, raw_clip):
    frames, raw = raw_clip
    r = subprocess.run([os.path.join(BIN, "vs_eval_jitter"), "--score", "flow", str(raw)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "Farneback" in r.stderr and "not OpenCV's binary" in r.stderr
    got = float(r.stdout.strip().split("\tmedian_jitter_px=")[1])
    want, _ = gpu_vs.flow_jitter(frames)
    assert want > 1.0
    assert "%g" % got == "%g" % want, (got, want)


def test_eval_jitter_default_is_the_similarity_score(gpu_vs, raw_clip):
    frames, raw = raw_clip
    default = subprocess.run([os.path.join(BIN, "vs_eval_jitter"), str(raw)], capture_output=True, text=True, timeout=600)
    explicit = subprocess.run([os.path.join(BIN, "vs_eval_jitter"), "--score", "similarity", str(raw)], capture_output=True, text=True,
                              timeout=600)
    assert default.returncode == 0 and explicit.returncode == 0
    assert default.stdout == explicit.stdout and default.stderr == explicit.stderr
    assert "Farneback flow, eval_jitter.cpp:43-70): it sees global camera motion only" in default.stderr
    bad = subprocess.run([os.path.join(BIN, "vs_eval_jitter"), "--score", "optical", str(raw)], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0


def test_grid_search_align_flow_score(gpu_vs, raw_clip):
    frames, raw = raw_clip
    out = run("vs_grid_search_align", raw, "-j", 2, "--frames", 12, "--score", "flow", "--dump-ratios")
    j_in = float(re.search(r"Input median jitter: (\S+) px", out).group(1))
    assert "%g" % j_in == "%g" % gpu_vs.flow_jitter(frames[:12])[0]
    ratios = re.findall(r"^RATIO (\d+) (\S+)$", out, re.M)
    assert len(ratios) == 54 and all(np.isfinite(float(v)) for _, v in ratios)
    assert re.search(r"Best params: .*ratio=", out)
