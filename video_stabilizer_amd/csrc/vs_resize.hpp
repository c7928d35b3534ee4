// vs_resize.hpp -- THE RESIZE RULE's tap tables (include/vs_amd.h: vs_bgr_resize_batch, vs_resize_taps), and the launch
// shape of the kernel that resamples with them.  Host and device, integers only, no HIP include: the table kernel and the launcher
// (vs_resize.hip), the host entry point vs_resize_taps (vs_capi_resize.hip) and tests/cpp/resize_rule_test.cpp all include this file, and the
// table rule is written nowhere else.
//
// A destination index d of an axis (source extent s, destination extent dn, each 1 .. 32767) gets a first source index i0, a count n >= 1 and
// weights wt[0 .. n) >= 0 that sum to 4096 exactly.
//
// LINEAR, any ratio.  With 64-bit integers num = (2 d + 1) s - dn and p = floor(num * 4096 / (2 dn)), floor towards minus infinity; p is
// clamped to [0, (s - 1) * 4096]; i = p >> 12, f = p & 4095.  The taps are (i, 4096 - f) and (min(i + 1, s - 1), f).  The second tap is
// listed only where f != 0 (then i + 1 <= s - 1: the clamp leaves f == 0 at i == s - 1), so n is 1 or 2 and no listed weight is 0.
//
// AREA, only where dn <= s <= 8 dn.  In units of 1 / dn source pixels, cell d covers [d s, (d + 1) s); its taps are the source pixels
// k = floor(d s / dn) .. floor(((d + 1) s - 1) / dn); cum_k = min((k + 1) dn, (d + 1) s) - d s, C_k = floor((cum_k * 4096 + floor(s / 2)) / s),
// wt_k = C_k - C_(k-1) with C = 0 in front of the first tap.  The last cum is s, so the weights sum to 4096; n <= floor(s / dn) + 2 <= 10.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VSR_HD __host__ __device__
#else
#define VSR_HD
#endif

namespace vsr {

constexpr int kLinear = 0, kArea = 1;                      // VS_RESIZE_LINEAR, VS_RESIZE_AREA
constexpr int kMaxTaps = 10, kOne = 4096, kMaxExtent = 32767;

// one axis: the extents, and the filter where it applies
VSR_HD inline bool resize_axis_valid(int s, int dn, int filter) {
    if (s < 1 || dn < 1 || s > kMaxExtent || dn > kMaxExtent) return false;
    if (filter == kLinear) return true;
    return filter == kArea && dn <= s && (long long)s <= 8LL * dn;
}
VSR_HD inline bool resize_params_valid(int sw, int sh, int dw, int dh, int filter) {
    return resize_axis_valid(sw, dw, filter) && resize_axis_valid(sh, dh, filter);
}

// destination index d of an axis s -> dn: *i0 and wt[0 .. n), returns n.  (resize_axis_valid(s, dn, filter), 0 <= d < dn)
VSR_HD inline int resize_taps_linear(int s, int dn, int d, int* i0, uint16_t* wt) {
    const long long num = (2LL * d + 1) * s - dn, den = 2LL * dn, a = num * kOne;
    long long p = a >= 0 ? a / den : -((-a + den - 1) / den);
    const long long top = (long long)(s - 1) * kOne;
    p = p < 0 ? 0 : (p > top ? top : p);
    const int f = (int)(p & (kOne - 1));
    *i0 = (int)(p >> 12);
    wt[0] = (uint16_t)(kOne - f);
    if (f == 0) return 1;
    wt[1] = (uint16_t)f;
    return 2;
}
VSR_HD inline int resize_taps_area(int s, int dn, int d, int* i0, uint16_t* wt) {
    const long long lo = (long long)d * s, hi = lo + s;
    const int k0 = (int)(lo / dn), k1 = (int)((hi - 1) / dn);
    long long before = 0;
    for (int k = k0; k <= k1; k++) {
        const long long edge = (long long)(k + 1) * dn, cum = (edge < hi ? edge : hi) - lo;
        const long long c = (cum * kOne + s / 2) / s;
        wt[k - k0] = (uint16_t)(c - before);
        before = c;
    }
    *i0 = k0;
    return k1 - k0 + 1;
}
VSR_HD inline int resize_taps(int s, int dn, int filter, int d, int* i0, uint16_t* wt) {
    return filter == kArea ? resize_taps_area(s, dn, d, i0, wt) : resize_taps_linear(s, dn, d, i0, wt);
}

// ---- the tables as the kernels read them -------------------------------------------------------------------------------------------
// kEntryWords dwords per destination index: i0 | n << 16, then the ten weights as uint16 pairs (unused ones 0).  The x axis' dw entries
// first, the y axis' dh entries behind them.
constexpr int kEntryWords = 1 + kMaxTaps / 2;
inline size_t resize_table_words(int dw, int dh) { return (size_t)kEntryWords * ((size_t)dw + (size_t)dh); }

// ---- the launch shape of vs_k_bgr_resize -------------------------------------------------------------------------------------------
// A workgroup owns kTileW destination columns by R destination rows and keeps H of every source row its R rows touch in LDS, a dword per
// (source row, channel, column).  source_rows_bound: no R consecutive destination rows touch more source rows than this --
//   LINEAR  the rows' centres lie (R - 1) s / dn apart, and a row takes floor(centre) and the row below: floor((R - 1) s / dn) + 3
//   AREA    rows floor(e s / dn) .. floor(((e + R) s - 1) / dn): floor((R s + dn - 2) / dn) + 1
// resize_tile_rows: the largest R of 16, 8, 4, 2, 1 whose bound fits kLdsRows rows (kLdsBytes of LDS); R = 1 always does (3 rows, or at
// the 8:1 limit 9).  tests/cpp/resize_rule_test.cpp holds the bound against the tables for every pair it admits.
constexpr int kTileW = 64, kMaxTileRows = 16;
constexpr int kLdsBytes = 48 * 1024, kLdsRowBytes = kTileW * 3 * 4, kLdsRows = kLdsBytes / kLdsRowBytes;      // 64 source rows
inline long long source_rows_bound(int s, int dn, int filter, int R) {
    return filter == kArea ? ((long long)R * s + dn - 2) / dn + 1 : ((long long)(R - 1) * s) / dn + 3;
}
inline int resize_tile_rows(int sh, int dh, int filter) {
    for (int R = kMaxTileRows; R > 1; R >>= 1)
        if (source_rows_bound(sh, dh, filter, R) <= kLdsRows) return R;
    return 1;
}

}  // namespace vsr
