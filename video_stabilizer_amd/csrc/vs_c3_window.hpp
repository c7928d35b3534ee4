// vs_c3_window.hpp -- the tile-window decision of the float-tile warps (vs_warp.hip: vs_k_bgr_warp_c3 in its four modes, vs_k_warp_c3_tables):
// does the source footprint of one output tile fit the staged window in LDS, where does that window lie, and can the sampler address it.  One
// copy: the kernel's in-tile geometry (with the frame's extents and from the tile's four corners) and the tables kernel call the same
// function, so a tabled launch and an untabled one take the same decision by construction; plain C++ that device and host compilers accept
// alike, so that the decision is tested on the host against the sampler's own positions, pixel by pixel (tests/cpp/c3_window_test.cpp,
// tests/test_c3_window_cpp.py).  Beside it, as plain host code, the two functions that prepare and read the frames' extents: c3_extents and
// c3_compact_shape.  No HIP builtins.  Every user compiles with -ffp-contract=off: each product and sum below rounds where it is written.
#pragma once

#include <algorithm>
#include <cmath>

#if defined(__HIPCC__)
#define VS_C3W_HD __host__ __device__ __forceinline__
#else
#define VS_C3W_HD inline
#endif

namespace vsd {

struct C3Window {
    bool fits;                  // the tile samples from the staged window; otherwise pixel by pixel from global memory
    int sx_lo, sy_lo;           // first staged column (a multiple of 4 pixels) and row, in source pixels
    int rows, groups;           // staged rows and column groups of 4 pixels (meaningful where fits)
};
struct C3Params { float A1, B, TX, TY; };                    // the kernel's {1 + A, B, TX, TY}: Wx = A1 x - B y + TX, Wy = B x + A1 y + TY
struct C3Extents { float lo_x, hi_x, lo_y, hi_y; };          // c3_extents' four numbers of the frame
struct C3Tile { int x0, y0, tile_w, tile_h; };               // the tile's origin in the output window, the kernel's tile
struct C3Roi { int x, y, w, h; };                            // the output window in the frame
// the staged window of the instantiation: its rows and column groups, the LDS row pitch in staged pixels, and org = 1 where the tap window
// starts one pixel up / left of floor() (the Lanczos2 forms' float tile), 0 on the bilinear mode's raw tile
struct C3Staged { int max_rows, max_groups, pitch, org; };

// with_extents: E holds the frame's extents (one evaluation at the tile origin plus four adds); otherwise the footprint comes from the tile's
// four corners (Wx = fl(fl(A1 x) - fl(B y)) + TX is monotone in x and in y: the extremes sit at corners chosen by the signs of A1 and B).
VS_C3W_HD C3Window c3_tile_window(C3Tile t, C3Roi roi, C3Params p, bool with_extents, C3Extents E, C3Staged s) {
    const float A1 = p.A1, B = p.B, TX = p.TX, TY = p.TY;
    const int x0 = t.x0, y0 = t.y0;
    const float fx0 = (float)(x0 + roi.x), fy0 = (float)(y0 + roi.y);
    float mnx, mxx, mny, mxy;
    if (with_extents) {
        const float Wx00 = A1 * fx0 - B * fy0 + TX, Wy00 = B * fx0 + A1 * fy0 + TY;
        mnx = Wx00 + E.lo_x; mxx = Wx00 + E.hi_x; mny = Wy00 + E.lo_y; mxy = Wy00 + E.hi_y;
    } else {
        const int x1 = (x0 + t.tile_w < roi.w ? x0 + t.tile_w : roi.w) - 1, y1 = (y0 + t.tile_h < roi.h ? y0 + t.tile_h : roi.h) - 1;
        const float fx1 = (float)(x1 + roi.x), fy1 = (float)(y1 + roi.y);
        const float xa = A1 >= 0.f ? fx0 : fx1, xb = A1 >= 0.f ? fx1 : fx0;     // x minimising / maximising A1*x
        const float ya = B >= 0.f ? fy0 : fy1, yb = B >= 0.f ? fy1 : fy0;       // y minimising / maximising B*y
        mnx = A1 * xa - B * yb + TX; mxx = A1 * xb - B * ya + TX;
        const float xc = B >= 0.f ? fx0 : fx1, xd = B >= 0.f ? fx1 : fx0;       // x minimising / maximising B*x
        const float yc = A1 >= 0.f ? fy0 : fy1, yd = A1 >= 0.f ? fy1 : fy0;
        mny = B * xc + A1 * yc + TY; mxy = B * xd + A1 * yd + TY;
    }
    bool fits = fmaxf(fmaxf(fabsf(mnx), fabsf(mxx)), fmaxf(fabsf(mny), fabsf(mxy))) < 1.0e6f;
    int sx_lo = 0, sy_lo = 0, rows = 0, groups = 0;
    if (fits) {
        sx_lo = ((int)floorf(mnx) - 1) & ~3;               // first staged column: a multiple of 4 pixels (12 bytes)
        const int sx_hi = (int)floorf(mxx) + 2;
        sy_lo = (int)floorf(mny) - 1;
        const int sy_hi = (int)floorf(mxy) + 2;
        rows = sy_hi - sy_lo + 1;
        groups = (sx_hi - sx_lo + 4) >> 2;                 // column groups of 4 pixels
        // THE SAMPLER'S OFFSET IS FP32.  A pixel at floor position (flx, fly) reads its taps from the staged pixel
        //     off = (fly - (sy_lo + org)) pitch + (flx - (sx_lo + org)),
        // which the sampler forms (scaled by the bytes of a staged pixel, a power of two: no rounding of its own) as
        //     c0 = -(float)I,  I = R + (sx_lo + org),  R = (sy_lo + org) pitch       once per lane
        //     q  = fma(flx, 1, c0)                                                   = fl(flx - I) = fl(d - R),  d = flx - (sx_lo + org)
        //     off = (int)fma(fly, pitch, q)                                          = fl(off): 0 <= off < max_rows pitch, exact whenever q is.
        // (int) -> float rounds once |I| > 2^24, and q -- of magnitude |R| give or take d, 0 <= d < 4 max_groups <= pitch -- rounds once
        // |d - R| > 2^24: at 2^24 the spacing of floats is 2, so the offset comes out a staged pixel off (two from 2^25, four from 2^26...),
        // a neighbouring pixel's taps, no memory fault.  |sy_lo| may reach 10^6 under the test above: R reaches 8.1 10^7 at a pitch of 81.
        // Both are exact when |I| <= 2^24 - pitch and |R| <= 2^24 - pitch; a window further out (source row 207 000 at a pitch of 81,
        // 230 000 at 73, 190 000 at the raw tile's 88 -- every tap of such a tile lies outside any frame the library accepts, so it samples
        // the border) is left to the per-pixel path, which addresses with integers.  One sign test on wave-uniform integers
        // (|R|, |I| < 10^8: no wrap).
        const int lim = (1 << 24) - s.pitch;
        const int R = (sy_lo + s.org) * s.pitch, I = R + (sx_lo + s.org);
        fits = (((s.max_groups - groups) | (s.max_rows - rows) | (lim - R) | (lim + R) | (lim - I) | (lim + I)) >= 0);
    }
    return C3Window{fits, sx_lo, sy_lo, rows, groups};
}

// The per-frame extents that c3_tile_window adds to the position of a tile's origin: for the kernel parameters P = {A, B, TX, TY} of a
// frame, {min, max of A1*i - B*j, min, max of B*i + A1*j} over i in [0, 63], j in [0, tile_h - 1], widened by eps = 2^-20 * M, M = a bound
// on every intermediate of the fp32 position arithmetic over the output window (the arithmetic makes four roundings of relative size 2^-24
// on values below M, for the pixel and for the tile origin: 8 * 2^-24 * M; eps doubles that and covers the adds), and rounded outward to float.
inline void c3_extents(const float* P4, int n_frames, C3Roi roi, int tile_w, int tile_h, float* E4) {
    for (int f = 0; f < n_frames; f++) {
        const double A1 = (double)(1.0f + P4[4 * f]), B = (double)P4[4 * f + 1], TX = (double)P4[4 * f + 2], TY = (double)P4[4 * f + 3];
        const double X = (double)(roi.x + roi.w) + 64.0, Y = (double)(roi.y + roi.h) + (double)tile_h;
        const double M = std::max(std::fabs(A1) * X + std::fabs(B) * Y + std::fabs(TX), std::fabs(B) * X + std::fabs(A1) * Y + std::fabs(TY)) + 1.0;
        const double eps = M * (1.0 / 1048576.0);
        const double ax = A1 * (tile_w - 1), bx = -B * (tile_h - 1), ay = B * (tile_w - 1), by = A1 * (tile_h - 1);
        const double lo_x = std::min(0.0, ax) + std::min(0.0, bx) - eps, hi_x = std::max(0.0, ax) + std::max(0.0, bx) + eps;
        const double lo_y = std::min(0.0, ay) + std::min(0.0, by) - eps, hi_y = std::max(0.0, ay) + std::max(0.0, by) + eps;
        const double v[4] = {lo_x, hi_x, lo_y, hi_y};
        for (int k = 0; k < 4; k++) {
            float q = (float)v[k];
            if (!std::isfinite(v[k]) || !std::isfinite(q)) q = (k & 1) ? 3.0e38f : -3.0e38f;      // (the |.| < 1e6 test then refuses the window)
            else if ((k & 1) ? (double)q < v[k] : (double)q > v[k]) q = std::nextafterf(q, (k & 1) ? INFINITY : -INFINITY);
            E4[4 * f + k] = q;
        }
    }
}

// -> 0: the standard window; 1: every frame's tile footprint stays under 16 source rows (E4 = c3_extents' output): the 20-row windows hold
// floor(max) - floor(min) + 4 <= 20 rows for every tile; 2: ... and under 65 source columns: floor(max) - floor(min) + 4 taps + 3 of alignment
// <= 72 = the 18 column groups of the seven-wave shape
inline int c3_compact_shape(const float* E4, int n_frames) {
    int shape = 2;
    for (int f = 0; f < n_frames; f++) {
        if (!((double)E4[4 * f + 3] - (double)E4[4 * f + 2] < 15.999)) return 0;
        if (!((double)E4[4 * f + 1] - (double)E4[4 * f + 0] < 64.99)) shape = 1;
    }
    return shape;
}

}  // namespace vsd
