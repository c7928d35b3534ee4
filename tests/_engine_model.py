"""The engine's model: the CPU oracle's Stabilizer frame by frame, and the engine's pass chain rebuilt in numpy around it, stated once.

state() after each process() gives T_i, its success flag and the accumulated correction of the frame just put out (measure()).  The
candidates of output frame k are the frames j = k+1 .., as far as every alignment on the way succeeded, with

    chain_j = compose(T_{k+1}, ..., T_j)                 # t_compose(t1, t2) = t1 then t2
    cand_t  = inverse(chain_j)                           # the look-ahead passes: deblur, denoise, rolling shutter (lookahead_candidates)
    F_j     = compose(inverse(chain_j), C_k)             # the fill: C_k = inverse(accum), what frame k itself is warped with (fill_candidates)

The passes, in the engine's order (engine_model):

    1. deblur            target: the input frame;       candidates: the input frames
    2. denoise           target: the deblurred frame;   candidates: the input frames
    3. rolling shutter   on the frame so far; the motion is candidate 1 of a look-ahead list, inverse(T_{k+1})
    4. plain warp, or the border fill with the frame so far as candidate 0 and the input frames behind it, optionally blended (the sums
       and the candidates are the input frames'; only the plain value is the frame so far)
    5. inpaint of what the fill leaves open in the output window
    6. crop

A new pre-warp pass goes between 3 and 4 of engine_model(), as one more `if`; its per-pass rule stays in its own _ref module, like the others'.
The passes behind the warp that are modelled at kernel level from the off-handle's own outputs (deflicker, sharpen, resize, scene cut, lens,
YCbCr) are not here.

Test infrastructure only: the only product code used is the host algebra (cv_inverse_matrix), handed in by the caller.
"""
import numpy as np

import _deblur_ref as DB
import _denoise_ref as DN
import _fill_blend_ref as FB
import _fill_ref as FR
import _rolling_ref as RS


def measure(O, frames, **params):
    """the oracle's Stabilizer over one clip -> (meas, succ, due, params): T_i and its success flag per input frame, and
    {k: (plain output frame k, accumulated correction it was warped with)}"""
    st = O.Stabilizer(**params)
    lag = st.params.lag
    meas, succ, due = [], [], {}
    for i in range(len(frames)):
        o = st.process(frames[i])
        m, a, s = st.state()
        meas.append(O.Transform.of(*m.tup()))
        succ.append(s)
        if o is not None:
            due[i - lag] = (o, O.Transform.of(*a.tup()))
    return meas, succ, due, st.params


def _chains(A, k, ahead, meas, succ):
    """(j, chain_j) for j = k+1 .. k+ahead, until an alignment failed.  A: the algebra (the oracle, or capi)"""
    chain = A.Transform.of()
    for j in range(k + 1, k + ahead + 1):               # (frame k + lag has arrived when frame k is put out: all of them exist)
        if j >= len(meas) or not succ[j]:
            break
        chain = A.t_compose(chain, meas[j])
        yield j, chain


def lookahead_candidates(A, k, ahead, meas, succ, mode="right"):
    """(cand_frame, cand_t) of output frame k, ahead + 1 entries (a list cut short ends in -1).  mode: "right"; "flip" = the chain
    un-inverted (the wrong direction)"""
    cf, ct = [k], [A.Transform.of()]
    for j, chain in _chains(A, k, ahead, meas, succ):
        cf.append(j)
        ct.append(chain if mode == "flip" else A.t_inverse(chain))
    while len(cf) < ahead + 1:
        cf.append(-1)
        ct.append(A.Transform.of())
    return cf, ct


def fill_candidates(A, k, ahead, meas, succ, Ck, flip=False):
    """(cand_frame, cand_t) of output frame k for the fill: frame k under Ck first; a list cut short is short.  flip: chain_j un-inverted
    (the wrong direction, for the direction test)"""
    cf, ct = [k], [Ck]
    for j, chain in _chains(A, k, ahead, meas, succ):
        cf.append(j)
        ct.append(A.t_compose(chain if flip else A.t_inverse(chain), Ck))
    return cf, ct


class Model:
    """outs {k: output frame k, cropped like the engine's}; pre {k: frame k after the pre-warp passes}; masks {k: (cov0, still_open), with
    the blend (cov0, still_open, band)} on the cropped window, where asked for"""
    def __init__(self):
        self.outs, self.pre, self.masks = {}, {}, {}


def engine_model(O, frames, *, cvinv=None, deblur=0, deblur_params=(2.0, 4.0), denoise=0, strength=24, rolling=0.0, fill=0, blend=None,
                 inpaint=None, mode="right", flip=False, pixels=None, bits=None, max_value=None, want_masks=False, **params):
    """the oracle's Stabilizer over one clip with the passes applied -> Model.  deblur, denoise, fill: frames ahead (0: off); deblur_params:
    (sensitivity, max_ratio); rolling: the readout share (0: off); blend: (feather, match) or None; inpaint: tests/_inpaint_ref.py's
    inpaint(window, keep mask) or None; cvinv: the host algebra's cv_inverse_matrix (default: the oracle's); mode: the look-ahead lists'
    direction, flip: the fill lists' (the direction tests); pixels: another clip of the same shape whose samples (and sums) are used under the
    transforms measured on `frames`.  The fill, the inpaint and the masks need the fixed-point bilinear warp"""
    n, h, w, _ = frames.shape
    if bits is None:
        bits = 8 if frames.dtype == np.uint8 else 10
    if max_value is None:
        max_value = (1 << bits) - 1
    if cvinv is None:
        cvinv = O.cv_inverse_matrix
    meas, succ, due, p = measure(O, frames, **params)
    crop = max(p.crop_pixels, 0)
    win = (slice(crop, h - crop), slice(crop, w - crop))
    pix = frames if pixels is None else pixels
    untouched = not deblur and not denoise and rolling == 0 and pixels is None      # candidate 0 is the frame the oracle warped
    filled = fill > 0 or blend is not None or inpaint is not None or want_masks
    assert not filled or p.warp_mode == O.WARP_BILINEAR_CV
    sharp = DB.sharpness_batch(pix, bits) if deblur else None
    sums = FB.channel_sums(pix) if blend is not None and blend[1] else None
    res = Model()
    for k, (plain, acc) in due.items():
        d = own = pix[k]
        if deblur:
            cf, ct = lookahead_candidates(O, k, deblur, meas, succ, mode)
            d = DB.deblur_frame(cvinv, pix, sharp, cf, ct, bits, max_value, *deblur_params)
        if denoise:
            cf, ct = lookahead_candidates(O, k, denoise, meas, succ, mode)
            d = DN.denoise_target(O, d, [(pix[f], t) for f, t in zip(cf[1:], ct[1:]) if f >= 0], bits, max_value, strength)
        if rolling != 0:
            cf, ct = lookahead_candidates(O, k, min(1, p.lag), meas, succ, mode)
            M = cvinv(ct[1], w, h) if len(cf) > 1 and cf[1] >= 0 else None      # (a failed alignment or lag 0: no motion known)
            d = RS.rolling_frame(d, M, rolling, max_value)
        res.pre[k] = d
        Ck = O.t_inverse(acc)
        if not filled:
            t = Ck if p.warp_mode == O.WARP_BILINEAR_CV else O.t_inverse(Ck)
            full = O.bgr_image_warp(d, t, p.warp_mode, border=p.warp_border, max_value=max_value)
        else:
            cf, ct = fill_candidates(O, k, fill, meas, succ, Ck, flip)
            if blend is not None:
                p0 = None if d is own else O.bgr_image_warp(d, Ck, O.WARP_BILINEAR_CV, border=p.warp_border, max_value=max_value)
                full, *masks = FB.blend_frame(O, pix, cf, ct, sums, blend[0], blend[1], p.warp_border, max_value, want_masks=True, plain=p0)
                keep = masks[0] & ~masks[2]                 # outside the band ...
            else:
                src = pix
                if d is not own:                            # (frame 0 of the stack: the frame so far; frame j + 1: input frame j)
                    src, cf = np.concatenate([d[None], pix]), [0] + [j + 1 for j in cf[1:]]
                full, *masks = FR.fill_frame(O, src, cf, ct, p.warp_border, max_value, want_masks=True)
                keep = masks[0]
            if untouched:                                   # ... the covered pixels are the plain output
                assert np.array_equal(np.where(keep[win][..., None], full[win], plain), plain), k
            if inpaint is not None:                         # (the window is the cropped frame: the push-pull sees nothing outside it)
                full = full.copy()
                full[win] = inpaint(full[win], ~masks[1][win])
            if want_masks:
                res.masks[k] = tuple(m[win] for m in masks)
        res.outs[k] = full[win]
    return res
