// vs_cover.hpp -- the block / strip walk and the rectangle test that the passes behind a VS_WARP_BILINEAR_CV warp share: the border fill
// (vs_fill.hip) and the coverage index of the inpaint (vs_inpaint.hip).  One copy, so that "candidate 0 covers this rectangle" is the same
// decision in both.  Device code; the host restatement of the test is vsi::cv_window_covered (vs_lookahead.hpp).
#pragma once

#include "vs_kernels.hpp"
#include "vs_device.hpp"

namespace vsd {

constexpr int FL_W = 64, FL_ROWS = 16, FL_WAVES = 4;      // a wave's strip: 64 columns x 16 rows; four strips stacked = a 64 x 64 tile
constexpr int FL_BLOCK = 256;                              // a workgroup's block of output pixels (a side): 4 x 4 tiles
static_assert(FL_BLOCK % FL_W == 0 && FL_BLOCK % (FL_ROWS * FL_WAVES) == 0, "whole tiles");

// candidate 0 (matrix M) covers every pixel of the nx x ny rectangle at (x0, y0) of the output window.  Every table term within 2^29: the sums
// cannot wrap, and with monotone terms the extremes of X and Y over the rectangle are sums of corner terms.
__device__ __forceinline__ bool cv_covers_rect(const double M[6], vsk::Roi roi, int x0, int y0, int nx, int ny, int w, int h) {
    const int fxA = x0 + roi.x, fxB = x0 + nx - 1 + roi.x, fyA = y0 + roi.y, fyB = y0 + ny - 1 + roi.y;
    const int adA = cv_delta(M[0], fxA), adB = cv_delta(M[0], fxB), bdA = cv_delta(M[3], fxA), bdB = cv_delta(M[3], fxB);
    const int XA = cv_row_origin(M[1], M[2], fyA), XB = cv_row_origin(M[1], M[2], fyB);
    const int YA = cv_row_origin(M[4], M[5], fyA), YB = cv_row_origin(M[4], M[5], fyB);
    const int lim = 1 << 29;
    // (-lim < term < lim asked of the terms as they stand: a delta that cvRound saturated to INT_MIN has no absolute value in int, and abs() would
    // hand it back negative -- "small".  Reached by a near-singular candidate 0 on a one-row window at frame row 0: tests/test_fill_hostile_gpu.py)
    const int lo = min(min(min(adA, adB), min(bdA, bdB)), min(min(XA, XB), min(YA, YB)));
    const int hi = max(max(max(adA, adB), max(bdA, bdB)), max(max(XA, XB), max(YA, YB)));
    const bool small = lo > -lim && hi < lim;
    const int mnX = min(XA, XB) + min(adA, adB), mxX = max(XA, XB) + max(adA, adB);
    const int mnY = min(YA, YB) + min(bdA, bdB), mxY = max(YA, YB) + max(bdA, bdB);
    // ((X0 + adelta) >> 5) >> 5 = (X0 + adelta) >> 10
    return small && (mnX >> 10) >= 0 && (mxX >> 10) + 1 <= w - 1 && (mnY >> 10) >= 0 && (mxY >> 10) + 1 <= h - 1;
}

}  // namespace vsd
