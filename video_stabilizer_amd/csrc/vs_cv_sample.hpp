// vs_cv_sample.hpp -- the device side that the look-ahead passes share (fill, deblur, denoise, deflicker, rolling shutter, lens remap, YCbCr, sharpen):
// VS_WARP_BILINEAR_CV's weights and blend, the two taps of a frame row in one unaligned load, sample j of a lane's packed dwords, and the wave's
// strip copy for a frame with nothing to do.  The sampler is the numerics contract of all those passes ("device side"): it
// is written here once, and a pass keeps only its own walk, pipeline and rule.  Everything is __forceinline__: a kernel's code is what it was
// with the copy it used to carry.  Device-only; -ffp-contract=off as in vs_device.hpp, so the fp32 blend rounds exactly as written.
#pragma once

#include "vs_device.hpp"

namespace vsd {

// ---- the weights -------------------------------------------------------------------------------------------------------------------
// 8-bit containers blend in int, 16-bit containers in fp32
template <typename T> struct Weight { typedef int type; };
template <> struct Weight<uint16_t> { typedef float type; };

// the four weight products a0 b0, a1 b0, a0 b1, a1 b1 of a position's fractions (they sum to 1024)
__device__ __forceinline__ void cv_products(CvPos p, int m[4]) {
    const int a1 = p.X & 31, b1 = p.Y & 31, a0 = 32 - a1, b0 = 32 - b1;
    m[0] = a0 * b0; m[1] = a1 * b0; m[2] = a0 * b1; m[3] = a1 * b1;
}
// the products as the blend takes them: as they are (8-bit), times 1 / 1024 in fp32 (16-bit)
template <typename T>
__device__ __forceinline__ void cv_weights(const int m[4], typename Weight<T>::type wt[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (sizeof(T) == 1) wt[k] = (typename Weight<T>::type)m[k];
        else wt[k] = (typename Weight<T>::type)((float)m[k] * (1.0f / 1024.0f));
    }
}
template <typename T>
__device__ __forceinline__ void cv_weights(CvPos p, typename Weight<T>::type wt[4]) {
    int m[4];
    cv_products(p, m);
    cv_weights<T>(m, wt);
}

// ---- the blend ---------------------------------------------------------------------------------------------------------------------
// One channel of the four taps v00, v01 (row sy at columns sx, sx + 1) and v10, v11 (row sy + 1 likewise).  8-bit: (sum + 512) >> 10; 16-bit: the
// fp32 sum in this order, cvRound, saturated to [0, maxv]
__device__ __forceinline__ uint32_t cv_blend1(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, const int wt[4], int) {
    return (uint32_t)(((int)v00 * wt[0] + (int)v01 * wt[1] + (int)v10 * wt[2] + (int)v11 * wt[3] + 512) >> 10);
}
__device__ __forceinline__ uint32_t cv_blend1(uint32_t v00, uint32_t v01, uint32_t v10, uint32_t v11, const float wt[4], int maxv) {
    const float sum = (float)v00 * wt[0] + (float)v01 * wt[1] + (float)v10 * wt[2] + (float)v11 * wt[3];
    return (uint32_t)min(max((int)rintf(sum), 0), maxv);
}
// the three channels of taps held in registers: t[0], t[1], t[2], t[3] = v00, v01, v10, v11
template <typename W>
__device__ __forceinline__ void cv_blend(const uint32_t t[4][3], const W wt[4], int maxv, uint32_t q[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) q[c] = cv_blend1(t[0][c], t[1][c], t[2][c], t[3][c], wt, maxv);
}

// VS_WARP_BILINEAR_CV's value at a position whose four taps lie inside the frame.  r0: the first tap, in the caller's address space (a plain
// pointer to T or a GPtr<T>: the loads stay what the caller's were)
template <typename T, typename P>
__device__ __forceinline__ void cv_sample_inside(P r0, int stride, CvPos p, int maxv, uint32_t q[3]) {
    typename Weight<T>::type wt[4];
    cv_weights<T>(p, wt);
    const P r1 = r0 + stride;
#pragma unroll
    for (int c = 0; c < 3; c++) q[c] = cv_blend1(r0[c], r0[c + 3], r1[c], r1[c + 3], wt, maxv);
}

// ---- the two taps of one frame row -----------------------------------------------------------------------------------------------------
// A byte gather per sample is twelve loads per pixel, and a pass is then bound by the rate at which a CU takes gather instructions; the six
// samples of a row's two taps are neighbours, so (WIDE: the row holds at least eight elements, w >= 3) they come as ONE unaligned load of eight
// elements whose start is pulled back from the row's end, and a shift puts tap c0 at the bottom.  Every byte read lies inside the row.
// In two steps: row_fetch issues the load and keeps what came as it came, row_unpack shifts and unpacks it into a[3], b[3].  Apart, so that a
// pipelined caller (vs_remap.hip) has the loads of all its pixels in flight before it unpacks the first.
//   sh: WIDE, the bits that put tap c0 at the bottom, 8 sizeof(T) (3 c0 - the load's first element): 0 .. 5 samples;
//   d1: the second tap's distance from the first in samples, 3 or (the clamp folded them) 0.
struct __attribute__((packed)) PackedU64 { uint64_t v; };
struct __attribute__((packed, aligned(2))) PackedU128 { uint64_t lo, hi; };
template <typename T, bool WIDE> struct RowRaw { uint32_t s[6]; };
template <> struct RowRaw<uint8_t, true> { uint64_t q; };
template <> struct RowRaw<uint16_t, true> { uint64_t lo, hi; };

// p: WIDE, the load's first element; else tap c0's first sample
__device__ __forceinline__ RowRaw<uint8_t, true> row_fetch(GPtr<uint8_t> p, int, RowRaw<uint8_t, true>*) {
    return RowRaw<uint8_t, true>{((const __attribute__((address_space(1))) PackedU64*)p)->v};
}
__device__ __forceinline__ RowRaw<uint16_t, true> row_fetch(GPtr<uint16_t> p, int, RowRaw<uint16_t, true>*) {
    const __attribute__((address_space(1))) PackedU128* const q = (const __attribute__((address_space(1))) PackedU128*)p;
    return RowRaw<uint16_t, true>{q->lo, q->hi};
}
template <typename T>
__device__ __forceinline__ RowRaw<T, false> row_fetch(GPtr<T> p, int d1, RowRaw<T, false>*) {
    RowRaw<T, false> r;
#pragma unroll
    for (int c = 0; c < 3; c++) { r.s[c] = p[c]; r.s[3 + c] = p[d1 + c]; }
    return r;
}
__device__ __forceinline__ void row_unpack(const RowRaw<uint8_t, true>& r, int sh, int d1, uint32_t a[3], uint32_t b[3]) {
    const uint64_t q = r.q >> sh;
    const uint64_t q1 = d1 ? q >> 24 : q;                 // (d1 == 3: sh <= 16, the second tap ends at byte 7 at the most)
#pragma unroll
    for (int c = 0; c < 3; c++) { a[c] = (uint32_t)(q >> (8 * c)) & 255u; b[c] = (uint32_t)(q1 >> (8 * c)) & 255u; }
}
__device__ __forceinline__ void row_unpack(const RowRaw<uint16_t, true>& r, int sh, int d1, uint32_t a[3], uint32_t b[3]) {
    const uint64_t lo = r.lo, hi = r.hi;                  // sh: 0 .. 80 bits
    // (lo, hi) >> sh, the low 96 bits
    const uint64_t m0 = sh >= 64 ? hi >> (sh - 64) : (sh ? (lo >> sh) | (hi << (64 - sh)) : lo);
    const uint64_t m1 = sh >= 64 ? 0 : hi >> sh;
    const uint64_t ta = m0, tb = d1 ? (m0 >> 48) | (m1 << 16) : m0;                   // (d1 == 3: sh <= 32, nothing above bit 127 is asked for)
#pragma unroll
    for (int c = 0; c < 3; c++) { a[c] = (uint32_t)(ta >> (16 * c)) & 65535u; b[c] = (uint32_t)(tb >> (16 * c)) & 65535u; }
}
template <typename T>
__device__ __forceinline__ void row_unpack(const RowRaw<T, false>& r, int, int, uint32_t a[3], uint32_t b[3]) {
#pragma unroll
    for (int c = 0; c < 3; c++) { a[c] = r.s[c]; b[c] = r.s[3 + c]; }
}

// ---- sample j of a lane's packed dwords (four 8-bit or two 16-bit samples per dword, as they lie in memory) ------------------------------
template <typename T>
__device__ __forceinline__ uint32_t px_get(const uint32_t* d, int j) {
    return sizeof(T) == 1 ? (d[j / 4] >> (8 * (j % 4))) & 255u : (d[j / 2] >> (16 * (j % 2))) & 65535u;
}
// (into cleared dwords; v inside T's range)
template <typename T>
__device__ __forceinline__ void px_put(uint32_t* o, int j, uint32_t v) {
    if (sizeof(T) == 1) o[j / 4] |= v << (8 * (j % 4)); else o[j / 2] |= v << (16 * (j % 2));
}

// ---- a frame with nothing to do ------------------------------------------------------------------------------------------------------
// the wave's nx x (y1 - y0) strip at (x0, y0) is copied, as dwords where both rows allow it and as bytes for the rest.  The bounds build
// checks every access under sites SITE0 (dword store), SITE0 + 1 (dword load), SITE0 + 2 (byte store), SITE0 + 3 (byte load): an offset within
// a frame lies below (h - 1) * stride + 3 w elements
template <typename T, int SITE0>
__device__ __forceinline__ void strip_copy(const T* __restrict__ src, T* __restrict__ dst, int w, int h, int src_stride, int dst_stride, int x0, int nx, int y0,
                                           int y1, int lane) {
    const size_t row_bytes = (size_t)nx * 3 * sizeof(T);
    const bool wide = (((uintptr_t)src | (uintptr_t)dst | ((size_t)src_stride * sizeof(T)) | ((size_t)dst_stride * sizeof(T)) | ((size_t)x0 * 3 * sizeof(T))) & 3) == 0;
    for (int y = y0; y < y1; y++) {
        const uint8_t* const sp = (const uint8_t*)(src + (size_t)y * (size_t)src_stride + (size_t)x0 * 3);
        uint8_t* const dp = (uint8_t*)(dst + (size_t)y * (size_t)dst_stride + (size_t)x0 * 3);
        size_t done = 0;
        if (wide) {
            const size_t nd = row_bytes / 4;
            for (size_t i = lane; i < nd; i += 64)
                ((uint32_t*)dp)[VS_IDX(i, ((long long)(h - 1) * dst_stride + 3LL * w - ((long long)y * dst_stride + 3LL * x0)) * (long long)sizeof(T) / 4, SITE0)] = ((const uint32_t*)sp)[VS_IDX(i, ((long long)(h - 1) * src_stride + 3LL * w - ((long long)y * src_stride + 3LL * x0)) * (long long)sizeof(T) / 4, SITE0 + 1)];
            done = nd * 4;
        }
        for (size_t i = done + lane; i < row_bytes; i += 64)
            dp[VS_IDX(i, ((long long)(h - 1) * dst_stride + 3LL * w - ((long long)y * dst_stride + 3LL * x0)) * (long long)sizeof(T), SITE0 + 2)] = sp[VS_IDX(i, ((long long)(h - 1) * src_stride + 3LL * w - ((long long)y * src_stride + 3LL * x0)) * (long long)sizeof(T), SITE0 + 3)];
    }
}

}  // namespace vsd
