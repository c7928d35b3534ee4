// vs_sharpen.hip -- phase-compensated sharpening behind VS_WARP_BILINEAR_CV.  A bilinear resample is a two-tap box filter per axis, [1 - f, f],
// whose blur depends on the sub-pixel phase f: none at f = 0, most at f = 1/2.  In stabilised video every pixel's phase drifts from frame to frame
// with the correction, so the output's sharpness pulses in time and, under a rotation, across the frame.  The warp's positions carry five fraction
// bits; the filter [1 - a/32, a/32] has variance a (32 - a) / 1024 pixel^2 and its second-order inverse is identity - (variance / 2) [1, -2, 1]: a
// five-point stencil whose two weights are known per pixel from the warp's own matrix.  A pass of its own: no existing kernel is touched.
//
// THE SHARPEN RULE (also include/vs_amd.h, vs_bgr_sharpen_batch).
//
// - Scope.  Interleaved BGR, every `VS_FMT_BGR*`, frames up to 32767 a side (`VS_ERR_UNSUPPORTED` beyond, as the fill).
// - Image and window.  The input is an image of `roi_w x roi_h` pixels.  It is the window `[roi_x, roi_x + roi_w) x [roi_y, roi_y + roi_h)` of a
//   `w x h` output frame that `VS_WARP_BILINEAR_CV` made under the forward transform `t`.  `(x, y)` below are full-frame coordinates, as in the fill.
// - Positions.  `X`, `Y` (int32, five fraction bits) and `sx = X >> 5`, `sy = Y >> 5` are the fill's, to the letter (vs_fill.hip):
//   `M = vs_cv_inverse_matrix(t)`; `cvRound` saturates to int32, NaN gives 0, and `+ 16` and `X0 + adelta` wrap.
//   `a = X & 31`, `b = Y & 31`, `va = a (32 - a)`, `vb = b (32 - b)`.  Both lie in 0 .. 256.
// - Covered.  A pixel is covered iff all four taps lie in the frame (the fill's candidate-0 rule): `0 <= sx`, `sx + 1 <= w - 1`, `0 <= sy`,
//   `sy + 1 <= h - 1`.
// - Eligible.  A pixel is eligible iff it is not on the window's outermost row or column, it is covered, and its four edge neighbours
//   `(x +- 1, y)` and `(x, y +- 1)` are covered.
// - Delta.  For an eligible pixel and each channel, with raw samples `c, l, r, u, d` (no clamp of the taps):
//   `num = strength * (va * (2c - l - r) + vb * (2c - u - d))`, `delta = (num + 16384) >> 15`, an arithmetic shift.
// - Output.  `out = c` if the pixel is not eligible or `delta == 0`.  Otherwise `out = clamp(c + delta, 0, max_value)`.
// - Strength.  `strength` is 1 .. 32 in sixteenths, default 16: the filter's own variance, the derivation above, not a tuned value.
// - Bound.  `|num| <= 32 * 512 * 131070 = 2 147 450 880 < 2^31 - 16384`, so int32 is enough throughout.
//
// Hence
//
// - (a) under the identity or any whole-pixel shift every pixel comes back bit for bit;
// - (b) a constant image, and an image linear in `x` and `y`, come back bit for bit under any map;
// - (c) pixels the frame's own source does not cover (border, fill, inpaint), and their edge neighbours, come back bit for bit;
// - (d) a sample above `max_value` is changed only where `delta != 0`;
// - (e) a NaN map gives `X = Y = 16 >> 5 = 0` everywhere: every pixel is covered and `va = vb = 0`, so the image comes back bit for bit.
//
// KERNEL.  vs_k_bgr_sharpen<T, PX>: one launch over all frames of a call (grid y = frame), out of place.  A wave owns a strip of 64 PX columns and
// SH_ROWS rows and keeps a three-row window of its columns in registers, so a source row is loaded once per strip plus two halo rows.  PX = 4:
// four pixels per lane on packed dwords (three dwords of 8-bit, six of 16-bit samples; rows of both surfaces on dwords and roi_w a multiple of
// 4); PX = 1: a pixel per lane, sample by sample, for every other shape.  Left and right neighbours of a lane's pixels come from the lanes beside
// it by cross-lane moves; lane 0 and lane 63 load the pixel beyond the wave's two ends with the row.  Coverage is arithmetic on the positions, no
// memory: a lane evaluates the column terms cvRound(M0 x 1024), cvRound(M3 x 1024) of its PX + 2 columns once per strip, lane r evaluates the row
// origins of the strip's row r - 1 and the wave reads them back (as vs_k_scene_stats does), and the covered bits of a row travel through the
// window with the row.  The matrices are read from device memory with scalar loads.  No LDS, no barrier, no scratch.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int SH_WAVES = 4, SH_ROWS = 8;                   // a wave's strip is 64 lanes wide and 8 rows high; four strips stacked make a workgroup's tile

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every global access of this file, sites 621-629: 621 the frame's matrix; 622 / 623 a
// row load's row and column offsets; 624 the column offset of the pixel beyond a wave's end; 625 / 626 the store's row and column offsets; 627 the
// frame of a load, 628 the frame of a store.  The extents are written inside the macros' arguments, which the regular build drops.

// what a lane holds of one row: PX = 4: the packed dwords of its four pixels as they lie in memory; PX = 1: its pixel's three samples
template <typename T, int PX> struct RowRegs { static constexpr int N = PX == 1 ? 3 : PX * 3 * (int)sizeof(T) / 4; uint32_t d[N]; };
template <typename T, int PX>
__device__ __forceinline__ uint32_t sh_get(const RowRegs<T, PX>& r, int j) { return PX == 1 ? r.d[j] : px_get<T>(r.d, j); }

// a pixel's three samples in two words, for the cross-lane moves
struct Px3 { uint32_t lo, hi; };
template <typename T> __device__ __forceinline__ Px3 px3_pack(uint32_t s0, uint32_t s1, uint32_t s2) {
    return sizeof(T) == 1 ? Px3{s0 | (s1 << 8) | (s2 << 16), 0u} : Px3{s0 | (s1 << 16), s2};
}
template <typename T> __device__ __forceinline__ uint32_t px3_get(Px3 p, int k) {
    return sizeof(T) == 1 ? (p.lo >> (8 * k)) & 255u : (k == 2 ? p.hi : (p.lo >> (16 * k)) & 65535u);
}
template <typename T> __device__ __forceinline__ Px3 px3_up(Px3 p) {          // the value of the lane below (lane 0: its own)
    return Px3{(uint32_t)__shfl_up((int)p.lo, 1), sizeof(T) == 1 ? 0u : (uint32_t)__shfl_up((int)p.hi, 1)};
}
template <typename T> __device__ __forceinline__ Px3 px3_down(Px3 p) {        // the value of the lane above (lane 63: its own)
    return Px3{(uint32_t)__shfl_down((int)p.lo, 1), sizeof(T) == 1 ? 0u : (uint32_t)__shfl_down((int)p.hi, 1)};
}

// window row j of a frame: the lane's columns, and -- lane 0: the pixel in front of the wave's first column, lane 63: the pixel behind its last --
// the pixel beyond the wave's end where the window has one
template <typename T, int PX>
__device__ __forceinline__ void sh_load_row(const T* __restrict__ fs, int j, int i0, int lane, vsk::Roi roi, int src_stride, RowRegs<T, PX>& r, Px3& halo) {
    const T* const row = fs + VS_IDX((size_t)j * (size_t)src_stride, (long long)(roi.h - 1) * src_stride + 1, 622);
#pragma unroll
    for (int k = 0; k < RowRegs<T, PX>::N; k++) r.d[k] = 0;
    halo = Px3{0u, 0u};
    if (i0 < roi.w) {                                      // (PX == 4: roi.w is a multiple of 4, a lane's group is inside the row or past it)
        const T* const p = row + VS_IDX((size_t)i0 * 3, 3LL * roi.w - (3 * PX - 1), 623);
        if (PX == 1) {
#pragma unroll
            for (int k = 0; k < 3; k++) r.d[k] = p[k];
        } else {
#pragma unroll
            for (int k = 0; k < RowRegs<T, PX>::N; k++) r.d[k] = ((const uint32_t*)p)[k];
        }
    }
    const int hx = lane == 0 ? i0 - 1 : i0 + PX;
    if ((lane == 0 || lane == 63) && hx >= 0 && hx < roi.w) {
        const T* const p = row + VS_IDX((size_t)hx * 3, 3LL * roi.w - 2, 624);
        halo = px3_pack<T>(p[0], p[1], p[2]);
    }
}

// the covered bits of full-frame row origin (X0, Y0) at the lane's columns i0 - 1 .. i0 + PX: bit k is column i0 - 1 + k
template <int PX>
__device__ __forceinline__ uint32_t sh_cover(int X0, int Y0, const int ad[PX + 2], const int bd[PX + 2], int w, int h) {
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < PX + 2; k++) m |= (cv_covers(cv_pos(X0, Y0, ad[k], bd[k]), w, h) ? 1u : 0u) << k;
    return m;
}

template <typename T, int PX>
__global__ __launch_bounds__(64 * SH_WAVES) void vs_k_bgr_sharpen(const T* __restrict__ src, size_t src_fs, int n, int w, int h, int src_stride, int maxv,
                                                                  const double* __restrict__ minv, int strength, vsk::Roi roi, T* __restrict__ dst,
                                                                  size_t dst_fs, int dst_stride, int tiles_x) {
    typedef RowRegs<T, PX> Row;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int i0 = txi * PX * 64 + PX * lane, j0 = (tyi * SH_WAVES + wv) * SH_ROWS;      // window coordinates
    if (j0 >= roi.h) return;                                                             // wave-uniform
    const int j1 = min(j0 + SH_ROWS, roi.h);
    const int f = (int)blockIdx.y;
    const double* const M = minv + VS_IDX((size_t)f * 6, 6LL * n - 5, 621);
    const double M0 = M[0], M1 = M[1], M2 = M[2], M3 = M[3], M4 = M[4], M5 = M[5];
    // the column terms of the lane's columns i0 - 1 .. i0 + PX, once per strip
    int ad[PX + 2], bd[PX + 2];
#pragma unroll
    for (int k = 0; k < PX + 2; k++) { ad[k] = cv_delta(M0, roi.x + i0 - 1 + k); bd[k] = cv_delta(M3, roi.x + i0 - 1 + k); }
    // the row origins of window rows j0 - 1 .. j1: lane r has row j0 - 1 + r's (r <= SH_ROWS + 1 < 64)
    const int X0l = cv_row_origin(M1, M2, roi.y + j0 - 1 + lane), Y0l = cv_row_origin(M4, M5, roi.y + j0 - 1 + lane);
    const T* const fs = src + (size_t)VS_IDX(f, n, 627) * src_fs;
    T* const fd = dst + (size_t)VS_IDX(f, n, 628) * dst_fs;

    Row up, cur, dn;
    Px3 halo_cur, halo_dn;
    uint32_t m_up = 0, m_cur, m_dn;
#pragma unroll
    for (int k = 0; k < Row::N; k++) up.d[k] = 0;
    if (j0 > 0) {
        Px3 unused;
        sh_load_row<T, PX>(fs, j0 - 1, i0, lane, roi, src_stride, up, unused);
        m_up = sh_cover<PX>(__builtin_amdgcn_readlane(X0l, 0), __builtin_amdgcn_readlane(Y0l, 0), ad, bd, w, h);
    }
    sh_load_row<T, PX>(fs, j0, i0, lane, roi, src_stride, cur, halo_cur);
    int X0c = __builtin_amdgcn_readlane(X0l, 1), Y0c = __builtin_amdgcn_readlane(Y0l, 1);
    m_cur = sh_cover<PX>(X0c, Y0c, ad, bd, w, h);
#pragma unroll 1
    for (int j = j0; j < j1; j++) {                        // (wave-uniform: every lane stays for the cross-lane moves)
        const int rn = __builtin_amdgcn_readfirstlane(j - j0 + 2);
        const int X0n = __builtin_amdgcn_readlane(X0l, rn), Y0n = __builtin_amdgcn_readlane(Y0l, rn);
        if (j + 1 < roi.h) {
            sh_load_row<T, PX>(fs, j + 1, i0, lane, roi, src_stride, dn, halo_dn);
            m_dn = sh_cover<PX>(X0n, Y0n, ad, bd, w, h);
        } else {
#pragma unroll
            for (int k = 0; k < Row::N; k++) dn.d[k] = 0;
            halo_dn = Px3{0u, 0u};
            m_dn = 0;
        }
        // the pixels beside the lane's own: the last pixel of the lane below, the first of the lane above, or what the wave's ends loaded
        Px3 lp = px3_up<T>(px3_pack<T>(sh_get<T, PX>(cur, 3 * PX - 3), sh_get<T, PX>(cur, 3 * PX - 2), sh_get<T, PX>(cur, 3 * PX - 1)));
        Px3 rp = px3_down<T>(px3_pack<T>(sh_get<T, PX>(cur, 0), sh_get<T, PX>(cur, 1), sh_get<T, PX>(cur, 2)));
        if (lane == 0) lp = halo_cur;
        if (lane == 63) rp = halo_cur;
        const bool row_in = j >= 1 && j <= roi.h - 2;
        uint32_t o[Row::N];
#pragma unroll
        for (int k = 0; k < Row::N; k++) o[k] = 0;
#pragma unroll
        for (int i = 0; i < PX; i++) {
            const CvPos p = cv_pos(X0c, Y0c, ad[i + 1], bd[i + 1]);
            const int a = p.X & 31, b = p.Y & 31, va = a * (32 - a), vb = b * (32 - b);
            const bool elig = row_in && i0 + i >= 1 && i0 + i <= roi.w - 2 && ((m_cur >> i) & 7u) == 7u && ((m_up >> (i + 1)) & 1u) && ((m_dn >> (i + 1)) & 1u);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int c = (int)sh_get<T, PX>(cur, 3 * i + k);
                const int l = (int)(i > 0 ? sh_get<T, PX>(cur, 3 * (i - 1) + k) : px3_get<T>(lp, k));
                const int r = (int)(i < PX - 1 ? sh_get<T, PX>(cur, 3 * (i + 1) + k) : px3_get<T>(rp, k));
                const int u = (int)sh_get<T, PX>(up, 3 * i + k), d = (int)sh_get<T, PX>(dn, 3 * i + k);
                const int num = strength * (va * (2 * c - l - r) + vb * (2 * c - u - d));   // |num| <= 2 147 450 880: the rule's bound
                const int delta = (num + 16384) >> 15;
                const uint32_t q = elig && delta != 0 ? (uint32_t)clampi(c + delta, 0, maxv) : (uint32_t)c;
                if (PX == 1) o[k] = q; else px_put<T>(o, 3 * i + k, q);
            }
        }
        if (i0 < roi.w) {
            T* const op = fd + VS_IDX((size_t)j * (size_t)dst_stride, (long long)(roi.h - 1) * dst_stride + 1, 625) + VS_IDX((size_t)i0 * 3, 3LL * roi.w - (3 * PX - 1), 626);
            if (PX == 1) {
#pragma unroll
                for (int k = 0; k < 3; k++) op[k] = (T)o[k];
            } else {
#pragma unroll
                for (int k = 0; k < Row::N; k++) ((uint32_t*)op)[k] = o[k];
            }
        }
        up = cur; cur = dn; m_up = m_cur; m_cur = m_dn; halo_cur = halo_dn; X0c = X0n; Y0c = Y0n;
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_sharpen)

namespace vsk {

hipError_t bgr_sharpen(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int bits, int max_value, const double* minv_dev,
                       int strength, Roi roi, void* dst, size_t dst_fs, int dst_stride, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (n_frames < 1 || w < 1 || h < 1 || w > 32767 || h > 32767 || strength < 1 || strength > 32) return hipErrorNotSupported;
    if (roi.x < 0 || roi.y < 0 || roi.w < 1 || roi.h < 1 || roi.w > w - roi.x || roi.h > h - roi.y || src_stride < 3 * roi.w || dst_stride < 3 * roi.w)
        return hipErrorNotSupported;
    const size_t esz = (size_t)bits / 8;
    // four pixels per lane on dwords where every row of both surfaces starts on a dword
    const bool x4 = roi.w % 4 == 0 && rows_on_dwords(src, (size_t)src_stride, src_fs, n_frames, esz) && rows_on_dwords(dst, (size_t)dst_stride, dst_fs, n_frames, esz);
    const int tw = x4 ? 4 * 64 : 64, th = SH_ROWS * SH_WAVES;
    const int tiles_x = (roi.w + tw - 1) / tw, tiles_y = (roi.h + th - 1) / th;
    for_frame_chunks(n_frames, [&](int f0, int nf) {       // gridDim.y limit
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * SH_WAVES);
        const char* sp = (const char*)src + (size_t)f0 * src_fs * esz;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        const double* mp = minv_dev + (size_t)f0 * 6;
#define VS_SH_LAUNCH(T, PX) hipLaunchKernelGGL((vs_k_bgr_sharpen<T, PX>), grid, block, 0, s, (const T*)sp, src_fs, nf, w, h, src_stride, max_value, mp, strength, roi, (T*)dp, dst_fs, dst_stride, tiles_x)
        if (x4 && bits == 16) VS_SH_LAUNCH(uint16_t, 4);
        else if (x4) VS_SH_LAUNCH(uint8_t, 4);
        else if (bits == 16) VS_SH_LAUNCH(uint16_t, 1);
        else VS_SH_LAUNCH(uint8_t, 1);
#undef VS_SH_LAUNCH
    });
    return hipGetLastError();
}

}  // namespace vsk
