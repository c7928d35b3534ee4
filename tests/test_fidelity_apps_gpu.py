"""-m gpu: apps/vs_eval_fidelity prints what the library's fidelity statistics give for the frames of a clip (consecutive frames, or frame by frame
against a reference clip), and the point of the score: a stabilized clip's consecutive frames are more alike than its input's."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_apps_gpu import BIN, ROOT, run  # noqa: E402

pytestmark = pytest.mark.gpu
W, H, N = 160, 128, 12


@pytest.fixture(scope="module")
def clips(gpu_vs, tmp_path_factory):
    """the shaken clip and its steady twin: the same scene under the same pan"""
    from video_stabilizer_amd import synth
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "apps"), "-s", "-j4"])
    d = tmp_path_factory.mktemp("fidelity_recordings")
    shaken, _ = synth.make_clip(W, H, N, 3, channels=3, pan=0.5, jitter_t=4.0)
    steady, _ = synth.make_clip(W, H, N, 3, channels=3, pan=0.5, jitter_t=0.0, jitter_b=0.0, jitter_a=0.0)
    paths = {}
    for name, f in (("shaken", shaken), ("steady", steady)):
        paths[name] = d / ("%s_%dx%d.bgr" % (name, W, H))
        f.tofile(paths[name])
    paths["small"] = d / "small_96x64.bgr"
    shaken[:, :64, :96].tofile(paths["small"])
    return shaken, steady, paths


def _means(vs, a, b, pairs):
    """the means the tool prints, from the python binding: summed in the pairs' order, as the tool sums them"""
    h, w = a.shape[1:3]
    sc = vs.fidelity_scores(vs.fidelity_stats_batch(a, b, pairs), w, h)
    n = float(len(pairs))
    return [sum(min(float(v), 100.0) for v in sc[:, 3]) / n, sum(min(float(v), 100.0) for v in sc[:, 4]) / n, sum(float(v) for v in sc[:, 5]) / n]


def _fields(out, path, keys):
    line, = [l for l in out.strip().splitlines() if l.startswith(str(path) + "\t")]
    got = dict(kv.split("=") for kv in line.split("\t")[1:])
    assert list(got) == list(keys), line
    return [got[k] for k in keys]


ITF_KEYS = ("itf_psnr_db", "itf_psnr_y_db", "itf_ssim")
REF_KEYS = ("psnr_db", "psnr_y_db", "ssim")


@pytest.mark.parametrize("inset,chunk", [(0, None), (16, None), (16, 5), (3, 2)])
def test_itf_fields_are_the_library_s(gpu_vs, clips, inset, chunk):
    """with and without --inset (3: no row of the image starts on a dword); --chunk 5 and 2: the last frame of a chunk is carried over to the next"""
    shaken, steady, paths = clips
    args = ["--inset", inset] + (["--chunk", chunk] if chunk else [])
    out = run("vs_eval_fidelity", *args, paths["shaken"], paths["steady"])
    pairs = [(i, i + 1) for i in range(N - 1)]
    for name, frames in (("shaken", shaken), ("steady", steady)):
        f = frames[:, inset:H - inset, inset:W - inset]
        want = _means(gpu_vs, f, None, pairs)
        assert _fields(out, paths[name], ITF_KEYS) == ["%g" % v for v in want], (name, want)
    sh, st = (list(map(float, _fields(out, paths[k], ITF_KEYS))) for k in ("shaken", "steady"))
    assert all(b > a for a, b in zip(sh, st))                           # the steady twin scores above the shaken clip in every field


def test_note_and_frames_option(gpu_vs, clips):
    shaken, steady, paths = clips
    r = subprocess.run([os.path.join(BIN, "vs_eval_fidelity"), "--frames", "5", str(paths["shaken"])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "inter-frame transformation fidelity" in r.stderr and "not equal to, what other tools print" in r.stderr
    assert _fields(r.stdout, paths["shaken"], ITF_KEYS) == ["%g" % v for v in _means(gpu_vs, shaken[:5], None, [(i, i + 1) for i in range(4)])]


def test_ref_fields_are_the_library_s(gpu_vs, clips):
    shaken, steady, paths = clips
    for args, inset in (([], 0), (["--inset", 16, "--chunk", 5], 16)):
        r = subprocess.run([os.path.join(BIN, "vs_eval_fidelity"), *map(str, args), "--ref", str(paths["steady"]), str(paths["shaken"]), str(paths["steady"])],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "against the same frame of the reference clip" in r.stderr
        a, b = (f[:, inset:H - inset, inset:W - inset] for f in (shaken, steady))
        want = _means(gpu_vs, a, b, [(i, i) for i in range(N)])
        assert _fields(r.stdout, paths["shaken"], REF_KEYS) == ["%g" % v for v in want]
        assert want[0] < 40.0 and want[2] < 0.95
        # a clip against itself
        assert _fields(r.stdout, paths["steady"], REF_KEYS) == ["100", "100", "1"]


def test_a_reference_of_another_size_is_an_error(gpu_vs, clips):
    shaken, steady, paths = clips
    r = subprocess.run([os.path.join(BIN, "vs_eval_fidelity"), "--ref", str(paths["small"]), str(paths["shaken"])], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "the reference clip is 96x64" in r.stderr and "psnr_db" not in r.stdout


@pytest.mark.parametrize("seed,n_frames", [(3, N), (4, N), (3, 40)])
def test_stabilizing_raises_the_inter_frame_fidelity(gpu_vs, seed, n_frames):
    """the shaken clip through a Stabilizer at default parameters (lag 10, crop 32): the output's ITF against the ITF of the same frames of the
    input, in the window the output shows.  12 frames leave two output frames, one pair; the 40-frame clip of the same kind leaves 29.
    Measured gains: DESIGN.md section 29"""
    from video_stabilizer_amd import synth
    vs = gpu_vs
    N = n_frames
    frames, _ = synth.make_clip(W, H, N, seed, channels=3, pan=0.5, jitter_t=4.0)
    stab = vs.Stabilizer(device=0)
    c = stab.params.crop_pixels
    outs = np.stack([o for o in (stab.process(f) for f in frames) if o is not None])
    n = outs.shape[0]
    assert n == N - stab.params.lag >= 2 and outs.shape[1:] == (H - 2 * c, W - 2 * c, 3)
    pairs = [(i, i + 1) for i in range(n - 1)]
    itf_out = _means(vs, outs, None, pairs)
    itf_in = _means(vs, frames[:n, c:H - c, c:W - c], None, pairs)
    print("seed %d: ITF in %.2f dB -> out %.2f dB (gray %.2f -> %.2f), SSIM %.4f -> %.4f over %d pairs"
          % (seed, itf_in[0], itf_out[0], itf_in[1], itf_out[1], itf_in[2], itf_out[2], len(pairs)))
    assert itf_out[0] > itf_in[0]
