"""vs_video_test with an output size (apps/vs_video_test.cpp: --out-size, --out-filter): the writer takes the delivered size, and the frames
it writes equal the library's resize of the plain run's frames."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 160, 128


def test_video_test_out_size_writes_the_resized_frames_of_the_plain_run(gpu_vs, tmp_path):
    vs = gpu_vs
    from video_stabilizer_amd import synth
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    frames = np.maximum(synth.make_clip(W, H, 20, seed=77, channels=3, pan=1.0, jitter_t=2.0)[0], 1)
    d = tmp_path / "in"
    d.mkdir()
    raw = d / ("shaky_%dx%d.bgr" % (W, H))
    frames.tofile(raw)
    exe = os.path.join(ROOT, "apps", "bin", "vs_video_test")

    def run(out, *args):
        r = subprocess.run([exe, str(d), str(tmp_path / out), "--crop", "16", "--chunk", "7", *args], capture_output=True, text=True, timeout=600)
        return r, tmp_path / out / ("processed_" + raw.name)
    r, path = run("plain")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    plain = np.fromfile(path, np.uint8).reshape(-1, H - 32, W - 32, 3)
    assert len(plain) > 0
    # the source size; a fixed size with the default filter (linear: no axis shrinks by more than 2:1; area: 128 -> 48 does) and a named one
    for args, (dw, dh), filt in ((["--out-size", "source"], (W, H), vs.RESIZE_LINEAR), (["--out-size", "96x64"], (96, 64), vs.RESIZE_LINEAR),
                                 (["--out-size", "48x40"], (48, 40), vs.RESIZE_AREA), (["--out-size", "96x64", "--out-filter", "area"], (96, 64), vs.RESIZE_AREA)):
        r, path = run("out_%dx%d_%d" % (dw, dh, filt), *args)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
        assert "Frame Size: %dx%d" % (dw, dh) in r.stdout
        got = np.fromfile(path, np.uint8).reshape(-1, dh, dw, 3)
        assert np.array_equal(got, vs.resize_batch(plain, dw, dh, filt)), args
    for args, word in ((["--out-size", "source", "--out-filter", "area"], "vs_stabilizer_process_batch"), (["--out-size", "40000x64"], "vs_stabilizer_set_output_size"),
                       (["--out-size", "96"], "--out-size takes"), (["--out-size", "96x64", "--out-filter", "cubic"], "--out-filter takes")):
        r, _ = run("bad", *args)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr[-500:])
