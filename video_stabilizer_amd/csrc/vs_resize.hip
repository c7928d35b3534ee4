// vs_resize.hip -- interleaved BGR frames from one size to another by THE RESIZE RULE (include/vs_amd.h: vs_bgr_resize_batch; the tap
// tables: vs_resize.hpp).  A pass of its own behind everything: no other kernel file is touched.
//
// SAMPLE.  v' = min(v, max_value).  Per channel H(y, d) = sum_k wx[d][k] * v'(y, ix0[d] + k), exact and below 2^28;
// V = sum_j wy[e][j] * H(iy0[e] + j, d), exact: it fits unsigned 32 bits for 8-bit frames with the rounding term
// (4096 * 4096 * 255 + 2^23 < 2^32), deeper frames take 64 bits; out = (V + 2^23) >> 24 -- one rounding per sample, here.  Every sum is an
// exact integer, so the order of the taps does not matter and both kernel forms below give the same bits.
//
// TABLES.  vs_k_resize_tables builds both axes' tables once per call (vsr::resize_taps, a thread per destination index): kEntryWords dwords
// per index, i0 | n << 16 and ten uint16 weights.  The frames of a call share them.
//
// vs_k_bgr_resize<T, X2> (the tiled form).  A workgroup of four waves owns 64 destination columns by R destination rows
// (vsr::resize_tile_rows) of one frame; frames go in gridDim.y, chunked at 65535.  A lane owns a column: it reads its x entry once.  Pass 1:
// the waves take the source rows the tile touches in turn and leave H of each in LDS, a dword per (row, channel, column) -- lane = column,
// so neither the stores nor the loads of pass 2 meet a bank conflict.  Pass 2: the waves take the destination rows in turn; the row's y entry
// is wave-uniform (scalar loads).  No scratch.
//
// TWO TAPS IN ONE LOAD (X2).  Where no x entry has more than two taps -- LINEAR at any ratio, AREA at 1:1 and 2:1 -- a lane reads a row's taps
// as one unaligned load of eight elements pulled back from the row's end, the remap's load (vs_cv_sample.hpp); else sample by sample.
//
// STORES.  A lane stores its pixel sample by sample.  Dword stores of a full tile's row, the lanes' pixels collected by wave shuffles, were
// built, gave the same bits and were 2 to 4 % slower on every shape measured: the stores do not bound these kernels.
//
// vs_k_bgr_resize_direct<T, X2> (the direct form).  The same tile of 64 columns by 4 rows, a row per wave; a lane gathers its nx * ny taps from
// memory and forms H per source row in registers.  No LDS, no barrier.
//
// WHICH FORM.  The tiled form where the frame grows in height (dh > sh): there destination rows share source rows and the tile forms H of
// each once.  The direct form otherwise: every source row belongs to one destination row, and the tile's barrier and LDS round trip buy
// nothing.  Measured both ways on three shapes, with registers, occupancy and how both stand against a plain copy: DESIGN.md section 30.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"
#include "vs_resize.hpp"

using namespace vsd;

namespace {

constexpr int RS_W = vsr::kTileW, RS_WAVES = 4, RS_EW = vsr::kEntryWords;

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every table, LDS, load and store offset of this file, sites 637-648: 637 a
// table entry's store; 638 / 639 the x and y entries' loads; 640 the frame; 641 / 642 a source row and a tap's (X2: the load's) column; 643 / 644 the LDS
// store and load of H; 645 / 646 the destination's row and column; 647 a y weight's load; 648 a y tap's source row.  The extents are written
// inside the macros' arguments, which the regular build drops.

template <typename T> struct Acc { typedef uint32_t type; };
template <> struct Acc<uint16_t> { typedef uint64_t type; };

__global__ __launch_bounds__(256) void vs_k_resize_tables(int sw, int dw, int sh, int dh, int filter, uint32_t* __restrict__ tab) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= dw + dh) return;
    const bool isx = i < dw;
    const int s = isx ? sw : sh, dn = isx ? dw : dh, d = isx ? i : i - dw;
    uint32_t* const e = tab + VS_IDX((size_t)i * RS_EW, (long long)(dw + dh - 1) * RS_EW + 1, 637);
    uint16_t* const wt = (uint16_t*)(e + 1);               // (weight k is the low or high half of word 1 + k / 2)
#pragma unroll
    for (int k = 0; k < vsr::kMaxTaps; k++) wt[k] = 0;
    int i0 = 0;
    const int n = vsr::resize_taps(s, dn, filter, d, &i0, wt);
    e[0] = (uint32_t)i0 | ((uint32_t)n << 16);
}

// A lane's x entry, kept in registers.  X2: no entry of the x table has more than two taps (LINEAR; AREA at 1:1 and 2:1) and a row holds
// eight elements.  Then both taps of a row come as ONE unaligned load of eight elements, pulled back from the row's end so that every byte
// read lies inside the row (vs_cv_sample.hpp: row_fetch, row_unpack, the remap's and the rolling-shutter pass's load): col the load's first
// element, sh the bits that put the first tap at the bottom, d1 the second tap's distance in samples (3, or 0 where there is none: its
// weight is 0).  Else the taps are read sample by sample.
template <bool X2> struct XTaps { int i0, n; uint32_t w[vsr::kMaxTaps / 2]; };
template <> struct XTaps<true> { int col, sh, d1; uint32_t w0, w1; };
template <typename T, bool X2>
__device__ __forceinline__ XTaps<X2> x_taps(const uint32_t* __restrict__ tab, int x, int dw, int sw) {
    XTaps<X2> t;
    const uint32_t* const e = tab + VS_IDX((size_t)x * RS_EW, (long long)(dw - 1) * RS_EW + 1, 638);
    const uint32_t h = e[0];
    const int i0 = (int)(h & 0xffffu), n = (int)(h >> 16);
    if constexpr (X2) {
        const uint32_t w = e[1];
        t.col = VS_IDX(min(3 * i0, 3 * sw - 8), 3LL * sw - 7, 642);
        t.sh = 8 * (int)sizeof(T) * (3 * i0 - t.col);     // (two taps: at most 2 samples; one tap: at most 5)
        t.d1 = n == 2 ? 3 : 0;
        t.w0 = w & 0xffffu; t.w1 = w >> 16;
    } else {
        t.i0 = i0; t.n = n;
#pragma unroll
        for (int k = 0; k < vsr::kMaxTaps / 2; k++) t.w[k] = e[1 + k];
    }
    return t;
}
// H of one source row at a lane's column, three channels (below 2^28).  Sample by sample the tap loop is unrolled over the ten possible taps
// with the count as a predicate, so that the weights are picked out of registers by constant indices.
template <typename T, bool X2>
__device__ __forceinline__ void h_sum(const T* __restrict__ row, const XTaps<X2>& t, int sw, uint32_t maxv, uint32_t h[3]) {
    if constexpr (X2) {
        uint32_t a[3], b[3];
        row_unpack(row_fetch((GPtr<T>)(row + t.col), t.d1, (RowRaw<T, true>*)nullptr), t.sh, t.d1, a, b);
#pragma unroll
        for (int c = 0; c < 3; c++) h[c] = t.w0 * min(a[c], maxv) + t.w1 * min(b[c], maxv);
    } else {
        h[0] = h[1] = h[2] = 0;
#pragma unroll
        for (int k = 0; k < vsr::kMaxTaps; k++) {
            if (k < t.n) {
                const uint32_t w = (t.w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
                const T* const p = row + VS_IDX((size_t)(t.i0 + k) * 3, 3LL * sw - 2, 642);
                h[0] += w * min((uint32_t)p[0], maxv); h[1] += w * min((uint32_t)p[1], maxv); h[2] += w * min((uint32_t)p[2], maxv);
            }
        }
    }
}
template <typename T>
__device__ __forceinline__ void put_pixel(T* __restrict__ o, const typename Acc<T>::type v[3]) {
    typedef typename Acc<T>::type A;
    o[0] = (T)((v[0] + ((A)1 << 23)) >> 24); o[1] = (T)((v[1] + ((A)1 << 23)) >> 24); o[2] = (T)((v[2] + ((A)1 << 23)) >> 24);
}

// tile_rows: vsr::resize_tile_rows(sh, dh, filter); lds_rows: the source rows the dynamic LDS holds (vsr::source_rows_bound of tile_rows)
template <typename T, bool X2>
__global__ __launch_bounds__(64 * RS_WAVES) void vs_k_bgr_resize(const T* __restrict__ src, size_t src_fs, int n, int sw, int sh, int src_stride, int maxv,
                                                                 const uint32_t* __restrict__ tab, T* __restrict__ dst, size_t dst_fs, int dw, int dh,
                                                                 int dst_stride, int tiles_x, int tile_rows, int lds_rows) {
    typedef typename Acc<T>::type A;
    extern __shared__ uint32_t rs_h[];                                     // [source row][channel][column]
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x = txi * RS_W + lane, e0 = tyi * tile_rows, e1 = min(e0 + tile_rows, dh);
    const bool live = x < dw;
    const size_t f = VS_IDX((size_t)blockIdx.y, n, 640);
    const uint32_t* const ytab = tab + (size_t)dw * RS_EW;
    // the source rows of the tile: from the first tap of its first row to the last tap of its last (both tables' i0 never decrease)
    const uint32_t ya = ytab[VS_IDX((size_t)e0 * RS_EW, (long long)(dh - 1) * RS_EW + 1, 639)];
    const uint32_t yb = ytab[VS_IDX((size_t)(e1 - 1) * RS_EW, (long long)(dh - 1) * RS_EW + 1, 639)];
    const int ys0 = (int)(ya & 0xffffu), nr = (int)(yb & 0xffffu) + (int)(yb >> 16) - ys0;
    XTaps<X2> xt{};
    if (live) xt = x_taps<T, X2>(tab, x, dw, sw);
    const T* const fsrc = src + f * src_fs;
    for (int r = wv; r < nr; r += RS_WAVES) {
        if (live) {
            uint32_t h[3];
            h_sum<T, X2>(fsrc + VS_IDX((size_t)(ys0 + r) * (size_t)src_stride, (long long)(sh - 1) * src_stride + 1, 641), xt, sw, (uint32_t)maxv, h);
#pragma unroll
            for (int c = 0; c < 3; c++) rs_h[VS_IDX((r * 3 + c) * RS_W + lane, (long long)lds_rows * 3 * RS_W, 643)] = h[c];
        }
    }
    __syncthreads();
    if (!live) return;
    for (int e = e0 + wv; e < e1; e += RS_WAVES) {
        const uint32_t* const ye = ytab + VS_IDX((size_t)e * RS_EW, (long long)(dh - 1) * RS_EW + 1, 639);
        const uint32_t hd = ye[0];
        const int r0 = (int)(hd & 0xffffu) - ys0, ny = (int)(hd >> 16);
        const uint16_t* const wy = (const uint16_t*)(ye + 1);
        A v[3] = {0, 0, 0};
        for (int j = 0; j < ny; j++) {
            const A w = (A)wy[VS_IDX(j, vsr::kMaxTaps, 647)];
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] += w * (A)rs_h[VS_IDX(((r0 + j) * 3 + c) * RS_W + lane, (long long)nr * 3 * RS_W, 644)];
        }
        put_pixel<T>(dst + f * dst_fs + VS_IDX((size_t)e * (size_t)dst_stride, (long long)(dh - 1) * dst_stride + 1, 645) + VS_IDX((size_t)x * 3, 3LL * dw - 2, 646), v);
    }
}

template <typename T, bool X2>
__global__ __launch_bounds__(64 * RS_WAVES) void vs_k_bgr_resize_direct(const T* __restrict__ src, size_t src_fs, int n, int sw, int sh, int src_stride, int maxv,
                                                                        const uint32_t* __restrict__ tab, T* __restrict__ dst, size_t dst_fs, int dw, int dh,
                                                                        int dst_stride, int tiles_x) {
    typedef typename Acc<T>::type A;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x = txi * RS_W + lane, e = tyi * RS_WAVES + wv;
    if (e >= dh || x >= dw) return;
    const size_t f = VS_IDX((size_t)blockIdx.y, n, 640);
    const XTaps<X2> xt = x_taps<T, X2>(tab, x, dw, sw);
    const uint32_t* const ye = tab + (size_t)dw * RS_EW + VS_IDX((size_t)e * RS_EW, (long long)(dh - 1) * RS_EW + 1, 639);
    const uint32_t hd = ye[0];
    const int iy0 = (int)(hd & 0xffffu), ny = (int)(hd >> 16);
    const uint16_t* const wy = (const uint16_t*)(ye + 1);
    const T* const fsrc = src + f * src_fs;
    A v[3] = {0, 0, 0};
    for (int j = 0; j < ny; j++) {
        const A w = (A)wy[VS_IDX(j, vsr::kMaxTaps, 647)];
        uint32_t h[3];
        h_sum<T, X2>(fsrc + (size_t)VS_IDX(iy0 + j, sh, 648) * (size_t)src_stride, xt, sw, (uint32_t)maxv, h);
#pragma unroll
        for (int c = 0; c < 3; c++) v[c] += w * (A)h[c];
    }
    put_pixel<T>(dst + f * dst_fs + VS_IDX((size_t)e * (size_t)dst_stride, (long long)(dh - 1) * dst_stride + 1, 645) + VS_IDX((size_t)x * 3, 3LL * dw - 2, 646), v);
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_resize)

namespace vsk {

size_t resize_table_ints(int dw, int dh) { return vsr::resize_table_words(dw, dh); }

hipError_t bgr_resize(const void* src, size_t src_fs, int n_frames, int sw, int sh, int src_stride, int bits, int max_value, int filter, int* tables,
                      void* dst, size_t dst_fs, int dw, int dh, int dst_stride, int form, hipStream_t s) {
    if (!container_ok(bits, max_value) || !vsr::resize_params_valid(sw, sh, dw, dh, filter)) return hipErrorNotSupported;
    if (n_frames < 1 || !src || !dst || !tables || src_stride < 3 * sw || dst_stride < 3 * dw) return hipErrorNotSupported;
    uint32_t* const tab = (uint32_t*)tables;
    hipLaunchKernelGGL(vs_k_resize_tables, dim3((unsigned)((dw + dh + 255) / 256)), dim3(256), 0, s, sw, dw, sh, dh, filter, tab);
    const size_t esz = (size_t)bits / 8;
    const int tiles_x = (dw + RS_W - 1) / RS_W;
    const int R = vsr::resize_tile_rows(sh, dh, filter), lds_rows = (int)std::min<long long>(vsr::source_rows_bound(sh, dh, filter, R), sh);
    if (form == kResizeAuto) form = dh > sh ? kResizeTiled : kResizeDirect;
    // both taps of a row in one load: no x entry has more than two, and a row holds the eight elements of the load
    const bool x2 = sw >= 3 && (filter == vsr::kLinear || sw == dw || sw == 2 * dw);
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const char* const sp = (const char*)src + (size_t)f0 * src_fs * esz;
        char* const dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        const dim3 block(64 * RS_WAVES);
        if (form == kResizeDirect) {
            const dim3 grid((unsigned)(tiles_x * ((dh + RS_WAVES - 1) / RS_WAVES)), (unsigned)nf);
#define VS_RS_LAUNCH(T, X2) hipLaunchKernelGGL((vs_k_bgr_resize_direct<T, X2>), grid, block, 0, s, (const T*)sp, src_fs, nf, sw, sh, src_stride, max_value, tab, (T*)dp, dst_fs, dw, dh, dst_stride, tiles_x)
            if (bits == 16) { if (x2) VS_RS_LAUNCH(uint16_t, true); else VS_RS_LAUNCH(uint16_t, false); }
            else { if (x2) VS_RS_LAUNCH(uint8_t, true); else VS_RS_LAUNCH(uint8_t, false); }
#undef VS_RS_LAUNCH
        } else {
            const dim3 grid((unsigned)(tiles_x * ((dh + R - 1) / R)), (unsigned)nf);
            const size_t lds = (size_t)lds_rows * vsr::kLdsRowBytes;
#define VS_RS_LAUNCH(T, X2) hipLaunchKernelGGL((vs_k_bgr_resize<T, X2>), grid, block, lds, s, (const T*)sp, src_fs, nf, sw, sh, src_stride, max_value, tab, (T*)dp, dst_fs, dw, dh, dst_stride, tiles_x, R, lds_rows)
            if (bits == 16) { if (x2) VS_RS_LAUNCH(uint16_t, true); else VS_RS_LAUNCH(uint16_t, false); }
            else { if (x2) VS_RS_LAUNCH(uint8_t, true); else VS_RS_LAUNCH(uint8_t, false); }
#undef VS_RS_LAUNCH
        }
    });
    return hipGetLastError();
}

}  // namespace vsk
