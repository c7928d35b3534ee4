// vs_rolling.hip -- rolling-shutter correction: a rolling-shutter sensor exposes a frame row by row, so camera motion shears and bends the frame
// from inside, which no transform per frame removes.  The pass resamples a frame so that every row shows what a global shutter would have
// shown at the frame's middle row time, from the motion to the FOLLOWING frame that the aligner has measured anyway.  A pass of its own in
// front of the warp: everything behind it (warp, fill, coverage index, inpaint, deflicker) sees a corrected frame and stays as it is.
//
// THE RULE (also include/vs_amd.h, vs_bgr_rolling_batch; DESIGN.md "Rolling-shutter correction").
// Interleaved BGR, every `VS_FMT_BGR*`, frames up to 32767 x 32767. Beyond that the call returns `VS_ERR_UNSUPPORTED`, as the denoise does.
//
// Inputs
//
// - Output frame `o` has exactly two candidate entries `(cand_frame, cand_t)`, laid out as in `vs_bgr_denoise_batch` with `n_cand == 2`.
// - Entry 0 is the frame to correct. Its transform is ignored.
// - Entry 1 carries the motion to the frame that follows it, in `VS_WARP_BILINEAR_CV`'s forward convention.
// - For entry 1 only the sign of `cand_frame` is looked at. That frame's pixels are never read.
// - A negative index means "no motion known".
// - `M[0..5] = vs_cv_inverse_matrix(cand_t[1], w, h)` is where pixel `(x, y)` of the frame lies in the following frame.
// - `readout` (`rho`) is the share of the frame period that the sensor takes to scan the frame from row 0 to row `h - 1`. Its range is
//   -1 .. 1; negative values mean bottom-up scanning. NaN or a value outside the range is `VS_ERR_ARG`.
//
// Row time
//
// `tau(y) = rho * ((double)(2 * y - (h - 1)) / (double)(2 * h))`.
//
// It is zero at the frame's middle. Every product and sum rounds once, in the order written: the build's `-ffp-contract=off`, no explicit FMA.
//
// Row matrix (fp64, same order)
//
// - `r0 = 1 + tau * (M0 - 1)`, `r1 = tau * M1`, `r2 = tau * M2`
// - `r3 = tau * M3`, `r4 = 1 + tau * (M4 - 1)`, `r5 = tau * M5`
//
// The row matrix is again of similarity form. The scene point that a global shutter would have shown at `(x, y)` sits in the raw frame at
// `r(y) * (x, y, 1)`. This is first order in the intra-frame motion.
//
// Position
//
// The position rule is `VS_WARP_BILINEAR_CV`'s own int32 rule, with the row's matrix in place of the frame's.
//
// - `X = (cv_row_origin(r1, r2, y) + cv_delta(r0, x)) >> 5`, `Y` likewise from `r4, r5, r3`. This is `cv_pos` of `vs_device.hpp`.
// - It keeps that rule's saturating `cvRound`, NaN -> 0, wrapping sums and arithmetic shifts.
// - The position has 5 fraction bits.
//
// Sample
//
// The blend is `VS_WARP_BILINEAR_CV`'s blend of the four taps at `(X >> 5, Y >> 5)` with fractions `X & 31`, `Y & 31`.
//
// - 8-bit containers: integer weights, `(sum + 512) >> 10`.
// - 16-bit containers: weights `a * b / 1024` in fp32, `rintf`, saturated to `vs_format_max_value(format)`.
// - Border: each tap's column is clamped to `0 .. w - 1` and its row to `0 .. h - 1`. The weights are unchanged.
// - No border colour can enter a corrected frame, so `warp_border` plays no part.
//
// Hence
//
// - (a) No motion: the frame comes back bit for bit, as a dword copy where the rows allow it.
// - (b) `rho == 0`: bit for bit.
// - (c) A motion of `{0, 0, 0, 0}`: bit for bit.
// - (d) For odd `h`, row `(h - 1) / 2` comes back bit for bit whatever the motion.
// - (e) Every output sample lies between the minimum and the maximum of the frame's samples in that channel.
// - (f) The rule defines every sample for every input the call accepts: NaN, singular and saturating matrices included.
// ((b) - (d): for samples up to the format's maximum and a finite motion -- the blend at zero fraction is the sample, which a 16-bit container
// then saturates, and tau * NaN is NaN whatever tau.)
//
// KERNEL.  vs_denoise.hip's shape: a wave owns a strip of columns and walks its rows; lane r evaluates tau, the two row origins and r0 / r3 of
// the strip's row r once, and the wave reads them with v_readlane (uniform values).  What is new: r0 and r3 depend on the row, so the two column
// cvRounds (fp64: two multiplies, rint, clamp, convert) are per pixel, not per strip; the rest per pixel is int32 -- position, clamped taps,
// fraction, blend -- plus the fp32 blend the 16-bit warp is defined by.  The frame and the matrix are scalar loads from the frame's two 64-byte
// entries (vsk::FillCand); the four taps are two GPtr gathers (global_load), one unaligned load of eight elements per frame row (row_fetch).  PX = 1: one pixel per
// lane, any width and pitch, a wave owns 64 columns x 8 rows.  PX = 4: a lane owns four consecutive pixels and stores them as three (u8) or six
// (u16) dwords, a wave owns 256 columns x 8 rows; for widths that are multiples of 4 with every destination row on a dword (the source is only
// gathered from: it needs no alignment).  A frame without motion is a copy, as dwords where both rows allow it.  No LDS, no barrier, no scratch.
// The pass moves one frame in and one frame out, and takes 2.3 times as long as the VS_WARP_BILINEAR_CV warp that moves the same bytes (32 4K
// frames: 0.72 ms 8-bit, 1.36 ms 10-bit, 0.28 of the HBM peak; DESIGN.md "Rolling-shutter correction").  What bounds it is vector-instruction issue,
// not bytes.  By the counters (rocprofv3 --pmc, 4K 8-bit, profiles/rolling_pmc.json): SQ_INSTS_VALU is 82 per pixel -- 14 of them fp64 by the assembly --
// against the warp's 34, a ratio of 2.41 where the kernel times stand 2.26 apart (695 us against 308 us); both kernels retire a vector instruction
// per SIMD every 4.6 - 4.9 cycles.  Loads are 2.0 per pixel (SQ_INSTS_VMEM_RD); the byte gathers of the first form, twelve per pixel, are gone.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int RS_W = 64, RS_WAVES = 4, RS_ROWS = 8;       // a wave's strip is 64 lanes wide and 8 rows high; four strips stacked make a workgroup's tile

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every gather and every store of this file, sites 581-590: an element offset within
// a frame, the access's last sample included, lies below (h - 1) * stride + 3 w (581-584 the copy, strip_copy<T, 581> of vs_cv_sample.hpp; 585 / 586 a gather's two row offsets, 587 / 588
// its two column offsets; 589 / 590 the store's row and column offsets).  The extents are written inside the macros' arguments, which the
// regular build drops.

// The two taps of one frame row: columns c0 and c1 (c1 == c0 + 1, or c1 == c0 where the clamp folded them) -> a[3], b[3].  WIDE: vs_cv_sample.hpp's
// row_fetch and row_unpack back to back, one unaligned load of eight elements pulled back from the row's end.  A row of fewer than eight
// elements is read sample by sample from its two taps' own addresses (the header's form with d1 costs this kernel two more subtractions).
template <bool WIDE, typename T>
__device__ __forceinline__ void rs_row_taps(GPtr<T> row, int w, int c0, int c1, uint32_t a[3], uint32_t b[3]) {
    if constexpr (WIDE) {
        const int e0 = c0 * 3, base = VS_IDX(min(e0, 3 * w - 8), 3LL * w - 7, 587), d1 = (c1 - c0) * 3;
        row_unpack(row_fetch(row + base, d1, (RowRaw<T, true>*)nullptr), 8 * (int)sizeof(T) * (e0 - base), d1, a, b);
    } else {
        GPtr<T> pa = row + VS_IDX(c0 * 3, 3LL * w - 2, 587), pb = row + VS_IDX(c1 * 3, 3LL * w - 2, 588);
#pragma unroll
        for (int c = 0; c < 3; c++) { a[c] = pa[c]; b[c] = pb[c]; }
    }
}
// the four taps of a position, columns and rows clamped into the frame: v[0], v[1] = row sy at columns sx, sx + 1; v[2], v[3] = row sy + 1 likewise
struct Taps { uint32_t v[4][3]; };
template <bool WIDE, typename T>
__device__ __forceinline__ Taps rs_taps(GPtr<T> fs, int w, int h, int stride, CvPos p) {
    const int sx = p.X >> 5, sy = p.Y >> 5;              // (|sx|, |sy| < 2^22: sx + 1 cannot overflow)
    const int c0 = clampi(sx, 0, w - 1), c1 = clampi(sx + 1, 0, w - 1);
    Taps t;
    rs_row_taps<WIDE>(fs + VS_IDX((size_t)clampi(sy, 0, h - 1) * (size_t)stride, (long long)(h - 1) * stride + 1, 585), w, c0, c1, t.v[0], t.v[1]);
    rs_row_taps<WIDE>(fs + VS_IDX((size_t)clampi(sy + 1, 0, h - 1) * (size_t)stride, (long long)(h - 1) * stride + 1, 586), w, c0, c1, t.v[2], t.v[3]);
    return t;
}
// VS_WARP_BILINEAR_CV's blend (vs_cv_sample.hpp) on those taps
template <typename T>
__device__ __forceinline__ void rs_blend(const Taps& t, CvPos p, int maxv, uint32_t q[3]) {
    typename Weight<T>::type wt[4];
    cv_weights<T>(p, wt);
    cv_blend(t.v, wt, maxv, q);
}

// cands: two entries per output frame (gridDim.y frames); entry 0 = the frame (its matrix is not read), entry 1 = the motion's output -> source
// matrix, a null frame there: no motion known.  PX: pixels per lane (1, or 4 with dword stores); WIDE: a row's two taps in one load (w >= 3)
template <typename T, int PX, bool WIDE>
__global__ __launch_bounds__(64 * RS_WAVES) void vs_k_bgr_rolling(const vsk::FillCand* __restrict__ cands, int w, int h, int src_stride, int maxv, double rho,
                                                                  T* __restrict__ dst, int dst_stride, size_t dst_fs, int tiles_x) {
    constexpr int R = RS_ROWS;
    constexpr int ND = PX * 3 * (int)sizeof(T) / 4;                       // dwords of a lane's four pixels (PX == 4)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x0 = txi * PX * RS_W, y0 = (tyi * RS_WAVES + wv) * R;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + R, h), nx = min(PX * RS_W, w - x0);
    cands += (size_t)blockIdx.y * 2;
    dst += (size_t)blockIdx.y * dst_fs;
    if (cands[1].src == nullptr) {                                        // uniform: no motion known
        strip_copy<T, 581>((const T*)cands[0].src, dst, w, h, src_stride, dst_stride, x0, nx, y0, y1, lane);
        return;
    }
    const GPtr<T> fs = (GPtr<T>)cands[0].src;
    const int x = min(x0 + PX * lane, w - PX);                            // (lanes past the row compute on its last group and store nothing)
    const bool lane_in = PX * lane < nx;
    // the row whose terms this lane evaluates: tau, the row matrix, the two row origins
    const int yl = y0 + (lane & (R - 1));
    const double tau = rho * ((double)(2 * yl - (h - 1)) / (double)(2 * h));
    const double r0l = 1.0 + tau * (cands[1].m[0] - 1.0), r3l = tau * cands[1].m[3];
    const int X0l = cv_row_origin(tau * cands[1].m[1], tau * cands[1].m[2], yl);
    const int Y0l = cv_row_origin(1.0 + tau * (cands[1].m[4] - 1.0), tau * cands[1].m[5], yl);
#pragma unroll 2
    for (int r = 0; r < R; r++) {
        if (y0 + r >= h) break;                                           // wave-uniform
        const int X0 = __builtin_amdgcn_readlane(X0l, r), Y0 = __builtin_amdgcn_readlane(Y0l, r);
        const double r0 = readlane_f64(r0l, r), r3 = readlane_f64(r3l, r);
        if (!lane_in) continue;
        T* const orow = dst + VS_IDX((size_t)(y0 + r) * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 589);
        if (PX == 1) {
            const CvPos pos = cv_pos(X0, Y0, cv_delta(r0, x), cv_delta(r3, x));
            uint32_t q[3];
            rs_blend<T>(rs_taps<WIDE>(fs, w, h, src_stride, pos), pos, maxv, q);
            T* const op = orow + VS_IDX((size_t)x * 3, 3LL * w - 2, 590);
            op[0] = (T)q[0]; op[1] = (T)q[1]; op[2] = (T)q[2];
        } else {
            uint32_t o[ND > 0 ? ND : 1];
#pragma unroll
            for (int k = 0; k < ND; k++) o[k] = 0;
#pragma unroll
            for (int i = 0; i < PX; i++) {
                const CvPos pos = cv_pos(X0, Y0, cv_delta(r0, x + i), cv_delta(r3, x + i));
                uint32_t q[3];
                rs_blend<T>(rs_taps<WIDE>(fs, w, h, src_stride, pos), pos, maxv, q);
#pragma unroll
                for (int k = 0; k < 3; k++) px_put<T>(o, 3 * i + k, q[k]);
            }
            uint32_t* const op = (uint32_t*)(orow + VS_IDX((size_t)x * 3, 3LL * w - (3 * PX - 1), 590));      // (3 PX samples)
#pragma unroll
            for (int k = 0; k < ND; k++) op[k] = o[k];
        }
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_rolling)

namespace vsk {

hipError_t bgr_rolling(const FillCand* cands_dev, int w, int h, int src_stride, int bits, int max_value, double readout, void* dst, int dst_stride,
                       int n_frames, size_t dst_fs, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (n_frames < 1 || w < 1 || h < 1 || w > 32767 || h > 32767 || !(readout >= -1.0 && readout <= 1.0)) return hipErrorNotSupported;
    const size_t esz = (size_t)bits / 8;
    // four pixels per lane with dword stores where every destination row starts on a dword
    const bool x4 = w % 4 == 0 && rows_on_dwords(dst, dst_stride, dst_fs, n_frames, esz);
    const int tw = x4 ? 4 * RS_W : RS_W, th = RS_ROWS * RS_WAVES;
    const int tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * RS_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * 2;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        // (the same arguments for every instantiation)
#define VS_RS_LAUNCH(T, PX, WIDE) hipLaunchKernelGGL((vs_k_bgr_rolling<T, PX, WIDE>), grid, block, 0, s, cp, w, h, src_stride, max_value, readout, (T*)dp, dst_stride, dst_fs, tiles_x)
        if (w < 3) { if (bits == 16) VS_RS_LAUNCH(uint16_t, 1, false); else VS_RS_LAUNCH(uint8_t, 1, false); }      // (a row of fewer than eight elements)
        else if (x4 && bits == 16) VS_RS_LAUNCH(uint16_t, 4, true);
        else if (x4) VS_RS_LAUNCH(uint8_t, 4, true);
        else if (bits == 16) VS_RS_LAUNCH(uint16_t, 1, true);
        else VS_RS_LAUNCH(uint8_t, 1, true);
#undef VS_RS_LAUNCH
    });
    return hipGetLastError();
}

}  // namespace vsk
