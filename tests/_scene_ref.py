"""The scene-cut rule (include/vs_amd.h: vs_bgr_scene_stats_batch, vs_scene_cuts) in numpy with Python integers for the sums, and the engine's
step with cuts (vs_stab_step.hpp: stab_step_cut) written with the C ABI's host algebra (vs_cv_inverse_matrix, vs_transform_*, the smoother).

    pair_stats / stats_batch      the lattice, the nearest-sample position, the clamped 8-bit levels, count and sad
    is_cut / cuts                 the decision, unsigned
    mean_level                    sad / (3 count): the mean absolute difference per sample, the figure the documents quote
    Step                          one stabilizer's bookkeeping, frame by frame: measurement, success, cut -> correction
    pair_transform                the pair's transform from the measurement T_j, as the look-ahead lists make candidate 1's

V: video_stabilizer_amd.capi (only its host-side functions are used: nothing here touches a device).  Test infrastructure only.
"""
from collections import deque

import numpy as np


def lattice_size(w, h, step):
    return -(-w // step) * -(-h // step)


def min_count(w, h, step):
    return max(1, lattice_size(w, h, step) // 16)


def pair_positions(V, t, w, h, step):
    """(qx, qy, inside) on the lattice for the FORWARD transform t: float64 (lh, lw), bool"""
    M = np.asarray(V.cv_inverse_matrix(t, w, h), np.float64).reshape(6)
    xs = np.arange(0, w, step, dtype=np.float64)[None, :]
    ys = np.arange(0, h, step, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        qx = np.rint((M[0] * xs + M[1] * ys) + M[2])
        qy = np.rint((M[3] * xs + M[4] * ys) + M[5])
        inside = np.isfinite(qx) & np.isfinite(qy) & (qx >= 0) & (qx <= w - 1) & (qy >= 0) & (qy <= h - 1)
    return qx, qy, inside


def pair_stats(V, target, cand, t, bits, step=4):
    """[count, sad] of one (target, candidate, t) pair, Python ints"""
    h, w, _ = target.shape
    s, maxv = bits - 8, (1 << bits) - 1
    qx, qy, inside = pair_positions(V, t, w, h, step)
    ix = np.where(inside, qx, 0).astype(np.int64)
    iy = np.where(inside, qy, 0).astype(np.int64)
    p = np.minimum(target[::step, ::step].astype(np.int64), maxv) >> s
    q = np.minimum(cand[iy, ix].astype(np.int64), maxv) >> s
    d = np.abs(p - q).sum(axis=-1)
    row = [int(inside.sum()), int(d[inside].sum())]
    assert row[0] < 2 ** 30 and row[1] < 3 * 255 * 2 ** 30               # the header's bounds
    return row


def stats_batch(V, src, pair_frames, pair_t, bits, step=4):
    """src (n_src, h, w, 3); pair_frames: (target, candidate) index pairs; pair_t: Transforms -> (n_pairs, 2) uint64"""
    rows = [pair_stats(V, src[int(a)], src[int(b)], t, bits, step) for (a, b), t in zip(pair_frames, pair_t)]
    return np.array(rows, np.uint64).reshape(-1, 2)


def is_cut(count, sad, w, h, step=4, threshold=32):
    count, sad = int(count), int(sad)
    return count < min_count(w, h, step) or sad > 3 * threshold * count


def cuts(stats, w, h, step=4, threshold=32):
    return np.array([is_cut(c, s, w, h, step, threshold) for c, s in np.asarray(stats, np.uint64).reshape(-1, 2).tolist()], np.uint8)


def mean_level(row):
    return row[1] / (3.0 * row[0]) if row[0] else float("inf")


def pair_transform(V, meas):
    """vs_lookahead.hpp over the single measurement T_j: inverse(compose(identity, T_j))"""
    return V.t_inverse(V.t_compose(V.Transform.of(), meas))


class Step:
    """stab_step_cut (vs_stab_step.hpp), call for call: the same host functions in the same order, so the same bits"""

    def __init__(self, V, params, w, h):
        self.V, self.p, self.w, self.h = V, params, w, h
        self.smoother = V.Smoother(params.lag, params.smoother_memory, params.lambda_)
        self.meas, self.ok, self.cut = deque(), deque(), deque()
        self.accum = V.Transform.of()

    def step(self, meas, success, cut):
        """-> None (nothing finalised) or the correction of the frame that left the queue"""
        V, p = self.V, self.p
        m = V.Transform.of() if cut else meas
        smoothed = V.Transform.of()
        if p.enable_smoother:
            _, smoothed = self.smoother.update(m)
        if not success:
            self.accum = V.Transform.of()
        self.meas.append(m)
        self.ok.append(1 if success and not cut else 0)
        self.cut.append(1 if cut else 0)
        if len(self.meas) <= p.lag:
            return None
        earliest, was_cut = self.meas.popleft(), self.cut.popleft()
        self.ok.popleft()
        if was_cut:
            self.accum = V.Transform.of()
            return V.t_inverse(self.accum)
        jitter = V.t_compose(earliest, V.t_inverse(smoothed)) if p.enable_smoother else earliest
        na = V.t_compose(self.accum, jitter)
        disp = V.t_max_corner_displacement(na, self.w, self.h)
        if disp > p.max_disp:
            decay = p.max_decay
        elif disp > p.min_disp:
            f = (disp - p.min_disp) / (p.max_disp - p.min_disp)
            f = max(0.0, min(1.0, f))
            decay = p.min_decay * (1.0 - f) + p.max_decay * f
        else:
            decay = p.min_decay
        na = V.Transform.of(na.A * decay, na.B * decay, na.TX * decay, na.TY * decay)
        self.accum = na
        return V.t_inverse(na)
