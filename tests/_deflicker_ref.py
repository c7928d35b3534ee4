"""The deflicker rule (include/vs_amd.h: vs_bgr_exposure_stats_batch, vs_exposure_gains_batch, vs_bgr_gain_batch) in numpy on top of the CPU
oracle's vs_cv_inverse_matrix, with Python integers for the sums and the divisions.

    pair_stats / stats_frame / stats_batch     the lattice, the nearest-sample position, the level test, the seven sums
    gains / gains_batch                        "used", the rounded Q15 ratio with its clamps, the rounded mean
    apply_gain / gain_batch                    the applied sample
    whole_frame_stats                          NOT the rule: whole-frame channel sums laid out as statistics, for the quality pin that shows why
                                               the rule measures at the same scene points
    window_gains                               the engine's candidate lists (tests/_engine_model.py's lookahead_candidates()) -> the gains of output frame k

Test infrastructure only: nothing of the product is used here.
"""
import numpy as np

from _engine_model import lookahead_candidates

UNIT = 32768


def lattice_size(w, h, step):
    return -(-w // step) * -(-h // step)


def threshold(w, h, step):
    return max(1, lattice_size(w, h, step) // 16)


def _level_ok(v, s):
    lv = v >> s
    return ((lv > 0) & (lv < 255)).all(axis=-1)


def pair_positions(O, t, w, h, step):
    """(qx, qy, inside) on the lattice for the FORWARD transform t: float64 (lh, lw), bool"""
    M = np.asarray(O.cv_inverse_matrix(t, w, h), np.float64).reshape(6)
    xs = np.arange(0, w, step, dtype=np.float64)[None, :]
    ys = np.arange(0, h, step, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.rint((M[0] * xs + M[1] * ys) + M[2])
        qy = np.rint((M[3] * xs + M[4] * ys) + M[5])
        inside = np.isfinite(qx) & np.isfinite(qy) & (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
    return qx, qy, inside


def pair_stats(O, target, cand, t, bits, step=4):
    """the eight words of one (target, candidate) pair: [count, a_B, a_G, a_R, b_B, b_G, b_R, 0], Python ints"""
    h, w, _ = target.shape
    s = bits - 8
    qx, qy, inside = pair_positions(O, t, w, h, step)
    ix = np.where(inside, qx, 0).astype(np.int64)
    iy = np.where(inside, qy, 0).astype(np.int64)
    p = target[::step, ::step].astype(np.int64)
    q = cand[iy, ix].astype(np.int64)
    ok = inside & _level_ok(p, s) & _level_ok(q, s)
    row = [int(ok.sum())] + [int(p[..., c][ok].sum()) for c in range(3)] + [int(q[..., c][ok].sum()) for c in range(3)] + [0]
    assert row[0] < 2 ** 30 and max(row[1:]) < 2 ** 46                   # the header's bounds
    return row


def stats_frame(O, src, cand_frame, cand_t, bits, step=4):
    """src (n_src, h, w, 3); cand_frame: indices (a negative one ends the list); cand_t: oracle Transforms (entry 0 is ignored).
    -> n_cand rows of eight Python ints; row 0 and the rows behind the list's end are zero"""
    assert cand_frame[0] >= 0
    rows = [[0] * 8 for _ in cand_frame]
    for j in range(1, len(cand_frame)):
        if int(cand_frame[j]) < 0:
            break
        rows[j] = pair_stats(O, src[int(cand_frame[0])], src[int(cand_frame[j])], cand_t[j], bits, step)
    return rows


def stats_batch(O, src, cand_frame, cand_t, bits, step=4):
    """-> (n_out, n_cand, 8) uint64"""
    return np.array([stats_frame(O, src, list(cf), list(ct), bits, step) for cf, ct in zip(cand_frame, cand_t)], np.uint64)


def ratio_q15(a, b):
    """clamp((2 * 32768 * b + a) / (2 * a), 16384, 65536), floor division; a == 0 (outside what the statistics can produce): 32768"""
    a, b = int(a), int(b)
    if a == 0:
        return UNIT
    assert 2 * UNIT * b + a < 2 ** 63
    return min(max((2 * UNIT * b + a) // (2 * a), 16384), 65536)


def gains(rows, w, h, step=4):
    """rows: n_cand rows of eight ints -> [G_B, G_G, G_R, m], Python ints"""
    thr = threshold(w, h, step)
    sums, m = [UNIT] * 3, 0
    for row in list(rows)[1:]:
        row = [int(v) for v in row]
        if row[0] < thr:
            continue
        m += 1
        for c in range(3):
            sums[c] += ratio_q15(row[1 + c], row[4 + c])
    return [(2 * sums[c] + (1 + m)) // (2 * (1 + m)) for c in range(3)] + [m]


def gains_batch(stats, w, h, step=4):
    """stats (n_out, n_cand, 8) -> (n_out, 4) uint32"""
    return np.array([gains(rows, w, h, step) for rows in np.asarray(stats).tolist()], np.uint32).reshape(-1, 4)


def apply_gain(frame, G, max_value):
    """min((v * G_c + 16384) >> 15, max_value); a frame with unit gains is left as it is, samples above the maximum included"""
    G = [int(g) for g in G[:3]]
    assert all(16384 <= g <= 65536 for g in G)
    if G == [UNIT] * 3:
        return frame.copy()
    v = frame.astype(np.int64) * np.array(G, np.int64)
    assert v.max() + 16384 < 2 ** 32
    return np.minimum((v + 16384) >> 15, max_value).astype(frame.dtype)


def gain_batch(src, G, max_value):
    return np.stack([apply_gain(f, g, max_value) for f, g in zip(src, np.asarray(G).tolist())])


def deflicker_frame(O, src, cand_frame, cand_t, bits, max_value, step=4):
    """statistics, gains and the applied frame of one output frame -> (frame, [G_B, G_G, G_R, m])"""
    _, h, w, _ = src.shape
    G = gains(stats_frame(O, src, cand_frame, cand_t, bits, step), w, h, step)
    return apply_gain(src[int(cand_frame[0])], G, max_value), G


def whole_frame_stats(src, cand_frame, step=4):
    """NOT the rule: every candidate's row from whole-frame channel sums (count = the lattice's size, so that it is used)"""
    _, h, w, _ = src.shape
    rows = [[0] * 8 for _ in cand_frame]
    tk = src[int(cand_frame[0])].astype(np.int64)
    for j in range(1, len(cand_frame)):
        if int(cand_frame[j]) < 0:
            break
        tj = src[int(cand_frame[j])].astype(np.int64)
        rows[j] = [lattice_size(w, h, step)] + [int(tk[..., c].sum()) for c in range(3)] + [int(tj[..., c].sum()) for c in range(3)] + [0]
    return rows


def window_gains(O, frames, k, ahead, meas, succ, bits, step=4, mode="right", whole=False):
    """the gains of output frame k from the window k .. k + ahead under the engine's candidate lists.  mode "flip": the chain un-inverted (the
    wrong direction); whole: whole-frame sums in place of the pair statistics"""
    _, h, w, _ = frames.shape
    cf, ct = lookahead_candidates(O, k, ahead, meas, succ, mode)
    rows = whole_frame_stats(frames, cf, step) if whole else stats_frame(O, frames, cf, ct, bits, step)
    return gains(rows, w, h, step)
