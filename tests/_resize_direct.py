"""The ideal THE RESIZE RULE approximates, in fractions.Fraction with no fixed-point weight anywhere: AREA is the exact box integral of the
source (pixel k covers [k, k + 1)) over the destination cell [d s / dn, (d + 1) s / dn), divided by the cell's length; LINEAR is exact linear
interpolation at the position ((2 d + 1) s - dn) / (2 dn), clamped to [0, s - 1].  Small frames only: every sample is a Fraction."""
from fractions import Fraction as Fr

LINEAR, AREA = 0, 1


def axis_weights(s, dn, filt, d):
    """-> {source index: exact weight}, the weights sum to 1"""
    if filt == AREA:
        lo, hi = Fr(d * s, dn), Fr((d + 1) * s, dn)
        out = {}
        k = int(lo)                                          # floor: lo >= 0
        while Fr(k) < hi:
            cover = min(Fr(k + 1), hi) - max(Fr(k), lo)
            if cover > 0:
                out[k] = cover / (hi - lo)
            k += 1
        return out
    c = min(max(Fr((2 * d + 1) * s - dn, 2 * dn), Fr(0)), Fr(s - 1))
    i = c.numerator // c.denominator
    f = c - i
    out = {i: 1 - f}
    if f:
        out[min(i + 1, s - 1)] = out.get(min(i + 1, s - 1), 0) + f
    return out


def resize(src, dw, dh, filt, max_value):
    """src (sh, sw, 3) array of ints -> nested lists [dh][dw][3] of Fractions: the unrounded ideal"""
    sh, sw = len(src), len(src[0])
    wx = [axis_weights(sw, dw, filt, d) for d in range(dw)]
    wy = [axis_weights(sh, dh, filt, e) for e in range(dh)]
    out = []
    for e in range(dh):
        row = []
        for d in range(dw):
            px = []
            for c in range(3):
                px.append(sum(ay * ax * min(int(src[y][x][c]), max_value) for y, ay in wy[e].items() for x, ax in wx[d].items()))
            row.append(px)
        out.append(row)
    return out
