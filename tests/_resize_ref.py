"""THE RESIZE RULE (include/vs_amd.h: vs_bgr_resize_batch, vs_resize_taps) restated in numpy.  The tap tables come from Python integers in this
file, not from the library; the sample sums are int64, which holds every value of the rule exactly (V + 2^23 <= 4096 * 4096 * 65535 + 2^23
< 2^41).  The restatement is independent of csrc/vs_resize.hpp: tests compare the two."""
import functools

import numpy as np

LINEAR, AREA = 0, 1
ONE = 4096
MAX_TAPS = 10

# the sweep of the table tests: every extent 1 .. 199 and the sizes a transcode meets
SWEEP_SIZES = list(range(1, 200)) + [1920, 3712, 3840, 32767]


def axis_valid(s, dn, filt):
    if not (1 <= s <= 32767 and 1 <= dn <= 32767):
        return False
    return filt == LINEAR or (filt == AREA and dn <= s <= 8 * dn)


def taps_linear(s, dn, d):
    """-> (i0, [weights])"""
    num = (2 * d + 1) * s - dn
    p = (num * ONE) // (2 * dn)                            # Python's // floors towards minus infinity
    p = min(max(p, 0), (s - 1) * ONE)
    i, f = p >> 12, p & 4095
    if f == 0:
        return i, [ONE]
    assert i + 1 <= s - 1
    return i, [ONE - f, f]


def taps_area(s, dn, d):
    lo, hi = d * s, (d + 1) * s
    k0, k1 = lo // dn, (hi - 1) // dn
    wt, before = [], 0
    for k in range(k0, k1 + 1):
        cum = min((k + 1) * dn, hi) - lo
        c = (cum * ONE + s // 2) // s
        wt.append(c - before)
        before = c
    return k0, wt


def taps(s, dn, filt, d):
    return taps_area(s, dn, d) if filt == AREA else taps_linear(s, dn, d)


@functools.lru_cache(maxsize=None)
def table(s, dn, filt):
    """the axis' table as vs_resize_taps returns it: (i0 (dn,) int32, n (dn,) int32, wt (dn, 10) uint16, unused weights 0)"""
    assert axis_valid(s, dn, filt), (s, dn, filt)
    i0 = np.zeros(dn, np.int32)
    n = np.zeros(dn, np.int32)
    wt = np.zeros((dn, MAX_TAPS), np.uint16)
    for d in range(dn):
        first, w = taps(s, dn, filt, d)
        i0[d], n[d] = first, len(w)
        wt[d, :len(w)] = w
    for a in (i0, n, wt):
        a.setflags(write=False)
    return i0, n, wt


def _axis_sum(v, s, dn, filt, axis):
    """sum_k wt[d][k] * v[.., i0[d] + k, ..] along `axis` (int64 in, int64 out)"""
    i0, n, wt = table(s, dn, filt)
    v = np.moveaxis(v, axis, 0)
    out = np.zeros((dn,) + v.shape[1:], np.int64)
    for k in range(int(n.max())):
        live = n > k
        idx = np.where(live, i0 + k, 0)
        w = np.where(live, wt[:, k].astype(np.int64), 0)
        out += w.reshape((-1,) + (1,) * (v.ndim - 1)) * v[idx]
    return np.moveaxis(out, 0, axis)


def resize(src, dw, dh, filt, max_value):
    """src (n, sh, sw, 3) uint8 / uint16 -> (n, dh, dw, 3) of the same dtype, by the rule"""
    src = np.asarray(src)
    n, sh, sw, c = src.shape
    v = np.minimum(src.astype(np.int64), max_value)
    H = _axis_sum(v, sw, dw, filt, 2)                       # (n, sh, dw, 3), below 2^28
    assert H.max(initial=0) < 1 << 28
    V = _axis_sum(H, sh, dh, filt, 1)
    return ((V + (1 << 23)) >> 24).astype(src.dtype)


def max_value_of(fmt_bits):
    return (1 << fmt_bits) - 1
