// vs_denoise.hip -- motion-compensated temporal denoise: a pixel is averaged with what other frames show at the same scene point, as far as they
// agree with it.  The stabilizer feeds it the input frames that FOLLOW the output frame: they are already held in device memory and their
// motions are already measured, so the samples of one scene point cost no second alignment, no frame storage and no latency.
//
// THE RULE (also include/vs_amd.h, vs_bgr_denoise_batch; DESIGN.md "Temporal denoise").  Interleaved BGR, every VS_FMT_BGR*, frames up to
// 32767 x 32767.
//   * CANDIDATES.  Output frame o has n_cand (1 .. 16) candidates (frame, forward transform t in VS_WARP_BILINEAR_CV's convention), exactly as
//     in vs_bgr_deblur_batch; candidate 0 is the target frame k itself (its transform is ignored); a candidate without a frame ends the list.
//   * SAMPLING.  The sample q_c of candidate j at target pixel (x, y) is, bit for bit, what vs_bgr_image_warp_roi_batch gives in mode
//     VS_WARP_BILINEAR_CV for that frame and transform with max_value = vs_format_max_value(format): cv::warpAffine's fixed-point bilinear
//     with the int32 positions of vs_fill.hip (cvRound saturated, NaN -> 0, wrapping sums, arithmetic shifts; 8-bit containers: integer
//     weights, (sum + 512) >> 10; 16-bit containers: the weights a b / 1024 in fp32, cvRound, saturated to max_value).  Candidate j takes part
//     at the pixel only if it COVERS it by the fill's rule: all four taps at the warp's own integer source position lie in the frame.  No
//     sample ever meets a border rule.  (Interpolation is wanted here, unlike in the deblur: a nearest sample leaves up to half a pixel of
//     misregistration, which an average turns into blur.)
//   * WEIGHTS AND OUTPUT.  Unsigned 32-bit integers throughout.  s = bits - 8; t = strength, 1 .. 255, in 8-bit levels;
//       d_j = max over the three channels of |p_c - q_c| >> s;      w_j = t - d_j if d_j < t, else 0
//       acc_c = t p_c + sum_j w_j q_c;      W = t + sum_j w_j
//     If sum_j w_j == 0 the pixel is p_c, bit for bit; otherwise it is min((2 acc_c + W) / (2 W), max_value), floor division.
//   * BOUND.  2 acc_c + W <= 2 * 16 * 255 * 65535 + 4080 < 2^30: every term fits, and the rule defines every sample for every input the API
//     accepts.
//   * HENCE (a) n_cand == 1, a list that ends at once and candidates that cover nothing give the frame back bit for bit; (b) identical
//     frames under identity maps come back bit for bit (the bilinear is exact at zero fraction, acc = W p); (c) |out_c - p_c| < t << s at
//     every pixel for any content and any maps (every contributing q_c lies that close to p_c, and the output is their weighted mean);
//     (d) a pixel whose candidates all differ from it by t levels or more in some channel is untouched.
//
// KERNELS.  adelta[x] / bdelta[x] of the warp's position depend on the column only, X0[y] / Y0[y] on the row only.  A lane keeps its columns
// while its wave walks a strip of rows with the candidate loop OUTSIDE the rows: per candidate and strip a lane evaluates the two column
// cvRounds (fp64) once, lane r evaluates the two row terms of the strip's row r once and the wave reads them with v_readlane (uniform
// values), and everything per pixel is int32 -- position, coverage, fraction, four taps, blend -- plus the fp32 blend the 16-bit warp is
// defined by.  The accumulators of the strip's rows stay in registers (the row loop is unrolled: static indices, no scratch).  The candidate
// loop is wave-uniform; matrices and frame pointers are scalar loads from a 64-byte entry per candidate (vsk::FillCand).  The one division
// per sample (2 acc + W < 2^30 by 2 W <= 8160) is a v_rcp_f32 estimate corrected by its remainder: the estimate's relative error is below
// 2^-21 and the quotient below 2^17, so it is off by at most one, which the remainder shows -- exact.  A frame with only candidate 0 is a
// dword copy.  vs_k_bgr_denoise: one sample per access, any width and pitch, a wave owns 64 columns x 8 rows.  vs_k_bgr_denoise_x4: a lane
// owns four consecutive pixels, the target read and the result stored as dwords, a wave owns 256 columns x 4 rows; for widths that are
// multiples of 4 with every target and destination row on a dword.  No LDS, no scratch, no barrier.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int DN_W = 64, DN_WAVES = 4;                    // a wave's strip is 64 lanes wide; four strips stacked make a workgroup's tile
constexpr int DN_ROWS = 8, DN_ROWS_X4 = 4;                // rows of a strip: per-sample kernel / four-pixel kernel

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every gather and every store of this file, sites 531-544: an element offset within
// a frame, the access's last sample included, lies below (h - 1) * stride + 3 w (531-534 the copy, strip_copy<T, 531> of vs_cv_sample.hpp; 535 / 541 the per-sample kernel's target row
// and column offsets, 536 its gathers, 537 / 542 its store's row and column offsets; 538 / 543, 539, 540 / 544 likewise in the four-pixel kernel).
// The extents are written inside the macros' arguments, which the regular build drops.

// one candidate at one pixel: p (the target's samples), acc / W (the sums so far)
template <typename T>
__device__ __forceinline__ void dn_take(GPtr<T> cs, int w, int h, int stride, CvPos pos, int maxv, int shift, uint32_t t, int site,
                                        const uint32_t p[3], uint32_t acc[3], uint32_t& W) {
    if (!cv_covers(pos, w, h)) return;
    uint32_t q[3];
    // (the four taps' last sample lies stride + 5 behind the first)
    cv_sample_inside<T>(cs + VS_IDX((size_t)(pos.Y >> 5) * (size_t)stride + (size_t)(pos.X >> 5) * 3, (long long)(h - 2) * stride + 3LL * w - 5, site), stride, pos, maxv, q);
    uint32_t d = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) d = max(d, (uint32_t)abs((int)p[c] - (int)q[c]));
    d >>= shift;
    if (d < t) {
        const uint32_t wt = t - d;
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] += wt * q[c];
        W += wt;
    }
}

// floor(n / d) for n < 2^30, 1 <= d <= 8160: the fp32 estimate is within one of the quotient (< 2^17), the remainder says which way
__device__ __forceinline__ uint32_t dn_div(uint32_t n, uint32_t d, float rd) {
    uint32_t q = (uint32_t)((float)n * rd);
    const int r = (int)n - (int)(q * d);
    if (r < 0) q--;
    else if (r >= (int)d) q++;
    return q;
}

// min((2 acc + W) / (2 W), maxv) per channel, or p where no candidate took part (W == t)
__device__ __forceinline__ void dn_finish(const uint32_t p[3], const uint32_t acc[3], uint32_t W, uint32_t t, uint32_t maxv, uint32_t out[3]) {
    const float rd = __builtin_amdgcn_rcpf((float)(2u * W));
#pragma unroll
    for (int c = 0; c < 3; c++) out[c] = W == t ? p[c] : min(dn_div(2u * acc[c] + W, 2u * W, rd), maxv);
}

// cands: n_cand entries per output frame (gridDim.y frames); entry 0 = the target frame (its matrix is not read), a null frame ends the list
template <typename T>
__global__ __launch_bounds__(64 * DN_WAVES) void vs_k_bgr_denoise(const vsk::FillCand* __restrict__ cands, int n_cand, int w, int h, int src_stride, int shift,
                                                                  int maxv, int strength, T* __restrict__ dst, int dst_stride, size_t dst_fs, int tiles_x) {
    constexpr int R = DN_ROWS;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x0 = txi * DN_W, y0 = (tyi * DN_WAVES + wv) * R;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + R, h), nx = min(DN_W, w - x0);
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    dst += (size_t)blockIdx.y * dst_fs;
    const T* const tgt = (const T*)cands[0].src;
    if (n_cand < 2 || cands[1].src == nullptr) {                          // uniform: only the frame itself
        strip_copy<T, 531>(tgt, dst, w, h, src_stride, dst_stride, x0, nx, y0, y1, lane);
        return;
    }
    const int x = min(x0 + lane, w - 1);                                  // (lanes past the row compute on its last column and store nothing)
    const bool lane_in = lane < nx;
    const uint32_t t = (uint32_t)strength;
    uint32_t p[R][3], acc[R][3], W[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int y = min(y0 + r, h - 1);                                 // (rows past the frame: read clamped, not stored)
        const T* const tp = tgt + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 535) + VS_IDX((size_t)x * 3, 3LL * w - 2, 541);
#pragma unroll
        for (int c = 0; c < 3; c++) { p[r][c] = tp[c]; acc[r][c] = t * p[r][c]; }
        W[r] = t;
    }
    const int yl = y0 + (lane & (R - 1));                                 // the row whose terms this lane evaluates
#pragma unroll 1
    for (int c = 1; c < n_cand; c++) {                                    // wave-uniform: the candidate's entry is read with scalar loads
        const GPtr<T> cs = (GPtr<T>)cands[c].src;
        if (!cs) break;
        const int ad = cv_delta(cands[c].m[0], x), bd = cv_delta(cands[c].m[3], x);
        const int X0l = cv_row_origin(cands[c].m[1], cands[c].m[2], yl), Y0l = cv_row_origin(cands[c].m[4], cands[c].m[5], yl);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (y0 + r >= h) break;                                       // wave-uniform
            const CvPos pos = cv_pos(__builtin_amdgcn_readlane(X0l, r), __builtin_amdgcn_readlane(Y0l, r), ad, bd);
            if (lane_in) dn_take(cs, w, h, src_stride, pos, maxv, shift, t, 536, p[r], acc[r], W[r]);
        }
    }
    if (!lane_in) return;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (y0 + r >= h) break;
        uint32_t o[3];
        dn_finish(p[r], acc[r], W[r], t, (uint32_t)maxv, o);
        T* const op = dst + VS_IDX((size_t)(y0 + r) * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 537) + VS_IDX((size_t)x * 3, 3LL * w - 2, 542);
        op[0] = (T)o[0]; op[1] = (T)o[1]; op[2] = (T)o[2];
    }
}

// The same pass for frames whose rows allow dword accesses on the target and the destination (w a multiple of 4; target frames, destination,
// rows and frame strides 4-byte aligned): a lane owns four consecutive pixels, reads them as three (u8) or six (u16) dwords and stores them
// likewise; the gathers stay per sample (a candidate's pixel lies anywhere).  The arithmetic per pixel is the kernel's above, operation for
// operation.  A wave owns 256 columns x 4 rows.
template <typename T>
__global__ __launch_bounds__(64 * DN_WAVES) void vs_k_bgr_denoise_x4(const vsk::FillCand* __restrict__ cands, int n_cand, int w, int h, int src_stride,
                                                                     int shift, int maxv, int strength, T* __restrict__ dst, int dst_stride, size_t dst_fs,
                                                                     int tiles_x) {
    constexpr int R = DN_ROWS_X4;
    constexpr int ND = 3 * (int)sizeof(T);                                // dwords of a lane's four pixels
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x0 = txi * 4 * DN_W, y0 = (tyi * DN_WAVES + wv) * R;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + R, h), nx = min(4 * DN_W, w - x0);
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    dst += (size_t)blockIdx.y * dst_fs;
    const T* const tgt = (const T*)cands[0].src;
    if (n_cand < 2 || cands[1].src == nullptr) {                          // uniform: only the frame itself
        strip_copy<T, 531>(tgt, dst, w, h, src_stride, dst_stride, x0, nx, y0, y1, lane);
        return;
    }
    const int x = min(x0 + 4 * lane, w - 4);                              // (lanes past the row compute on its last group and store nothing)
    const bool lane_in = 4 * lane < nx;
    const uint32_t t = (uint32_t)strength;
    uint32_t d[R][ND], acc[R][12], W[R][4];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int y = min(y0 + r, h - 1);
        const uint32_t* const tp = (const uint32_t*)(tgt + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 538) + VS_IDX((size_t)x * 3, 3LL * w - 11, 543));      // (twelve samples)
#pragma unroll
        for (int k = 0; k < ND; k++) d[r][k] = tp[k];
#pragma unroll
        for (int k = 0; k < 12; k++) acc[r][k] = t * px_get<T>(d[r], k);
#pragma unroll
        for (int i = 0; i < 4; i++) W[r][i] = t;
    }
    const int yl = y0 + (lane & (R - 1));
#pragma unroll 1
    for (int c = 1; c < n_cand; c++) {                                    // wave-uniform
        const GPtr<T> cs = (GPtr<T>)cands[c].src;
        if (!cs) break;
        const double m0 = cands[c].m[0], m3 = cands[c].m[3];
        int ad[4], bd[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { ad[i] = cv_delta(m0, x + i); bd[i] = cv_delta(m3, x + i); }
        const int X0l = cv_row_origin(cands[c].m[1], cands[c].m[2], yl), Y0l = cv_row_origin(cands[c].m[4], cands[c].m[5], yl);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (y0 + r >= h) break;                                       // wave-uniform
            const int X0 = __builtin_amdgcn_readlane(X0l, r), Y0 = __builtin_amdgcn_readlane(Y0l, r);
            if (lane_in) {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    uint32_t p[3];
#pragma unroll
                    for (int k = 0; k < 3; k++) p[k] = px_get<T>(d[r], 3 * i + k);
                    dn_take(cs, w, h, src_stride, cv_pos(X0, Y0, ad[i], bd[i]), maxv, shift, t, 539, p, &acc[r][3 * i], W[r][i]);
                }
            }
        }
    }
    if (!lane_in) return;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (y0 + r >= h) break;
        uint32_t o[ND];
#pragma unroll
        for (int k = 0; k < ND; k++) o[k] = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t p[3], v[3];
#pragma unroll
            for (int k = 0; k < 3; k++) p[k] = px_get<T>(d[r], 3 * i + k);
            dn_finish(p, &acc[r][3 * i], W[r][i], t, (uint32_t)maxv, v);
#pragma unroll
            for (int k = 0; k < 3; k++) px_put<T>(o, 3 * i + k, v[k]);
        }
        uint32_t* const op = (uint32_t*)(dst + VS_IDX((size_t)(y0 + r) * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 540) + VS_IDX((size_t)x * 3, 3LL * w - 11, 544));
#pragma unroll
        for (int k = 0; k < ND; k++) op[k] = o[k];
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_denoise)

namespace vsk {

hipError_t bgr_denoise(const FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int shift_to_8, int max_value, int strength, void* dst,
                       int dst_stride, int n_frames, size_t dst_fs, bool targets_aligned, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (shift_to_8 < 0 || shift_to_8 > 8 || n_cand < 1 || n_cand > 16 || n_frames < 1 || w < 1 || h < 1 || w > 32767 || h > 32767) return hipErrorNotSupported;
    if (strength < 1 || strength > 255) return hipErrorNotSupported;
    const size_t esz = (size_t)bits / 8;
    // four pixels per lane with dword accesses where every target row and every destination row starts on a dword
    const bool x4 = targets_aligned && w % 4 == 0 && rows_on_dwords(nullptr, src_stride, 0, 1, esz) && rows_on_dwords(dst, dst_stride, dst_fs, n_frames, esz);
    const int tw = x4 ? 4 * DN_W : DN_W, th = (x4 ? DN_ROWS_X4 : DN_ROWS) * DN_WAVES;
    const int tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * DN_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * (size_t)n_cand;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        if (x4 && bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_denoise_x4<uint16_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, shift_to_8, max_value, strength, (uint16_t*)dp,
                               dst_stride, dst_fs, tiles_x);
        else if (x4)
            hipLaunchKernelGGL(vs_k_bgr_denoise_x4<uint8_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, shift_to_8, max_value, strength, (uint8_t*)dp,
                               dst_stride, dst_fs, tiles_x);
        else if (bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_denoise<uint16_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, shift_to_8, max_value, strength, (uint16_t*)dp,
                               dst_stride, dst_fs, tiles_x);
        else
            hipLaunchKernelGGL(vs_k_bgr_denoise<uint8_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, shift_to_8, max_value, strength, (uint8_t*)dp,
                               dst_stride, dst_fs, tiles_x);
    });
    return hipGetLastError();
}

}  // namespace vsk
