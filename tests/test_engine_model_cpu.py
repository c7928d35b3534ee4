"""The unified engine model (tests/_engine_model.py) pinned to tests/golden/engine_model_digests.json: one SHA-256 per case over the outputs,
the frames after the pre-warp passes and the fill's masks, recorded from the five per-feature models this one replaced (the fill's, the
blend's, deblur's, denoise's and the rolling shutter's) when they were merged.  A pass moved in the order, a chain composed the other way
round or a candidate list that ends elsewhere changes a digest.  No GPU: the oracle and the host algebra (cv_inverse_matrix) only."""
import hashlib
import json
import os

import numpy as np
import pytest

import _deblur_ref as DB
import _engine_model as EM
import _inpaint_ref as IP

W, H, LAG = 160, 128, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_model_digests.json")
# one case per former model, each with the fill behind it, and every pass at once; the model's keywords apart from cvinv and inpaint
CASES = {"fill": dict(fill=3, want_masks=True),
         "fill_flip_10bit": dict(fill=3, want_masks=True, flip=True),
         "blend": dict(fill=3, blend=(4, 1), want_masks=True),
         "deblur": dict(deblur=3, fill=2),
         "denoise": dict(deblur=2, denoise=3, fill=2),
         "rolling": dict(rolling=0.8, fill=3),
         "all": dict(deblur=3, denoise=3, rolling=0.8, fill=3, inpaint=True)}
_clips = {}


def clip(bits=8):
    """14 frames of 160 x 128: rotation jitter, noise of 1 level, an exposure that drifts by +-10 %, two frames motion-blurred, no zero sample,
    and two frames in the middle that jump 40 px sideways and back: the alignment fails going in and coming out"""
    if bits not in _clips:
        from video_stabilizer_amd import synth
        a = DB.blurred_clip(synth, W, H, 12, 11, (3, 9), bits=bits, jitter_b=0.02)[0]
        a = np.concatenate([a[:6], np.roll(a[6:8], 40, axis=2), a[6:]])
        g = 1.0 + 0.1 * np.sin(2 * np.pi * np.arange(len(a)) / 7.0)
        _clips[bits] = np.clip(np.rint(a * g[:, None, None, None]), 1, (1 << bits) - 1).astype(a.dtype)
    return _clips[bits]


def case_inputs(name):
    """(frames, the model's keywords without cvinv and with inpaint still a flag)"""
    return clip(10 if name.endswith("10bit") else 8), dict(CASES[name], lag=LAG, crop_pixels=0)


def digest(outs, pre, masks):
    """outs, pre: {k: frame}; masks: {k: tuple of bool arrays} or empty"""
    d = hashlib.sha256()
    for k in sorted(outs):
        for a in (outs[k], pre[k]) + tuple(masks.get(k, ())):
            a = np.ascontiguousarray(a)
            d.update(("%d %s %s " % (k, a.dtype.str, a.shape)).encode())
            d.update(a.tobytes())
    return d.hexdigest()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_gives_what_the_five_models_gave(oracle, vs, name):
    O = oracle
    frames, kw = case_inputs(name)
    meas, succ, due, _ = EM.measure(O, frames, lag=LAG, crop_pixels=0)
    assert not all(succ[1:]), "the jump no longer makes an alignment fail: the test input has to change"
    short = [k for k in due if len(EM.fill_candidates(O, k, kw["fill"], meas, succ, O.Transform.of())[0]) < kw["fill"] + 1]
    assert short and len(short) < len(due), "no fill list is cut short (or every one is): the test input has to change"
    if kw.pop("inpaint", False):
        kw["inpaint"] = IP.inpaint
    m = EM.engine_model(O, frames, cvinv=lambda t, w, h: vs.cv_inverse_matrix(vs.Transform.of(*t.tup()), w, h), **kw)
    assert sorted(m.outs) == sorted(m.pre) == sorted(due) and len(due) == len(frames) - LAG
    assert sorted(m.masks) == (sorted(due) if kw.get("want_masks") else [])
    with open(GOLDEN) as f:
        assert digest(m.outs, m.pre, m.masks) == json.load(f)[name]
