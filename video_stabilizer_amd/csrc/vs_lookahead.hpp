// vs_lookahead.hpp -- the candidate transforms of the stabilizer's look-ahead passes (border fill, deblur, denoise, deflicker).  Host only, no HIP.
#pragma once

#include "../../include/vs_amd.h"

#include <stddef.h>
#include <algorithm>
#include <cmath>

namespace vsi {

// Frame k leaves the queue; the queue now holds the frames k+1 .. behind it and meas[c] is the motion T_{k+1+c} (T_j: frame j-1 to j), entry
// for entry, with ok[c] its alignment's success.  Frame k+1+c shows frame k's pixels through inverse(T_{k+1} o .. o T_{k+1+c}); with a
// `correction` (the fill: what frame k itself is warped by) it shows the OUTPUT through compose(that, correction).  The list ends at the first
// of: n_ahead entries, `avail` queued frames, a failed alignment.  out[0 .. n_ahead): the live entries, then {0, 0, 0, 0}.  Returns the live count.
// Meas / Ok: anything indexable (the engine's deques, arrays).  The arithmetic is these calls in this order -- the translation units are built
// with -ffp-contract=off, so every caller gets the same bits.
template <typename Meas, typename Ok>
inline int lookahead_transforms(const Meas& meas, const Ok& ok, size_t avail, int n_ahead, const vs_transform* correction, vs_transform* out) {
    vs_transform chain{0, 0, 0, 0};
    int live = 0;
    for (; live < n_ahead && (size_t)live < avail && ok[live]; live++) {
        chain = vs_transform_compose(&chain, &meas[live]);
        const vs_transform back = vs_transform_inverse(&chain);
        out[live] = correction ? vs_transform_compose(&back, correction) : back;
    }
    for (int c = live; c < n_ahead; c++) out[c] = vs_transform{0, 0, 0, 0};
    return live;
}

// ---- "candidate 0 covers the whole window", decided on the host: the int32 rectangle test of vs_cover.hpp (cv_covers_rect) restated, term for
// term, on the output -> source matrix M (vs_cv_inverse_matrix) and the window (rx, ry, rw, rh) of a w x h frame.  The same double
// operations in the same order (no contraction), cvRound = rint in the default rounding mode: the same ints as the device's.
inline int cv_round_sat_host(double v) {
    if (!(v == v)) return 0;
    return (int)std::fmin(std::fmax(std::rint(v), -2147483648.0), 2147483647.0);
}
inline int cv_delta_host(double m, int x) { return cv_round_sat_host(m * (double)x * 1024.0); }
inline int cv_row_origin_host(double my, double mt, int y) { return (int)((unsigned)cv_round_sat_host((my * (double)y + mt) * 1024.0) + 16u); }
inline bool cv_window_covered(const double M[6], int rx, int ry, int rw, int rh, int w, int h) {
    const int fxA = rx, fxB = rx + rw - 1, fyA = ry, fyB = ry + rh - 1;
    const int adA = cv_delta_host(M[0], fxA), adB = cv_delta_host(M[0], fxB), bdA = cv_delta_host(M[3], fxA), bdB = cv_delta_host(M[3], fxB);
    const int XA = cv_row_origin_host(M[1], M[2], fyA), XB = cv_row_origin_host(M[1], M[2], fyB);
    const int YA = cv_row_origin_host(M[4], M[5], fyA), YB = cv_row_origin_host(M[4], M[5], fyB);
    const int lim = 1 << 29;
    const int lo = std::min({adA, adB, bdA, bdB, XA, XB, YA, YB}), hi = std::max({adA, adB, bdA, bdB, XA, XB, YA, YB});
    if (!(lo > -lim && hi < lim)) return false;
    const int mnX = std::min(XA, XB) + std::min(adA, adB), mxX = std::max(XA, XB) + std::max(adA, adB);
    const int mnY = std::min(YA, YB) + std::min(bdA, bdB), mxY = std::max(YA, YB) + std::max(bdA, bdB);
    return (mnX >> 10) >= 0 && (mxX >> 10) + 1 <= w - 1 && (mnY >> 10) >= 0 && (mxY >> 10) + 1 <= h - 1;
}

}  // namespace vsi
