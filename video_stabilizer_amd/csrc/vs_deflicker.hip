// vs_deflicker.hip -- deflicker: a frame's exposure is pulled to the average exposure of the frames that follow it.  Auto-exposure and mains-lit
// scenes make the level of successive frames jump; a steady picture shows the jumps as pumping.  The stabilizer feeds this file the input frames
// that FOLLOW the output frame: they are already held in device memory and their motions are already measured, so the exposure ratio of two frames
// is taken at the SAME SCENE POINTS (a pan changes a whole-frame sum because the content changes; an overlap sum does not care), without a second
// alignment, frame storage, latency or a visit to the host.
//
// THE RULE (also include/vs_amd.h, vs_bgr_exposure_stats_batch; DESIGN.md "Deflicker").  Interleaved BGR, every VS_FMT_BGR*, frames up to
// 32767 a side; s = bits - 8.
//   * CANDIDATES.  Output frame o has n_cand (1 .. 16) candidates (frame, forward transform t in VS_WARP_BILINEAR_CV's convention), exactly as in
//     vs_bgr_denoise_batch; candidate 0 is the target frame k itself (its transform is ignored); a candidate without a frame ends the list.
//   * LATTICE.  step is 1 .. 64 (default 4); the lattice pixels are those with x % step == 0 && y % step == 0; L = ceil(w / step) * ceil(h / step).
//   * PAIR STATISTICS of candidate j >= 1.  With M = vs_cv_inverse_matrix(t_j) lattice pixel (x, y) lies in candidate j at
//     qx = rint((M0 x + M1 y) + M2), qy = rint((M3 x + M4 y) + M5): doubles, that order, no fma, ties to even -- the deblur's nearest-sample
//     position.  The pair COUNTS iff qx, qy are finite, 0 <= qx <= w - 1, 0 <= qy <= h - 1 and every one of the six samples v (three of p = the
//     target at (x, y), three of q = the candidate at (qx, qy)) has 0 < (v >> s) < 255: neither black nor clipped at 8-bit precision (this also
//     rejects samples above the format's maximum).  Per candidate seven uint64: count, a_c = sum p_c, b_c = sum q_c (count < 2^30, sums < 2^46;
//     integer sums: the order of the reduction cannot matter).  A NaN or infinite map counts nothing.
//   * GAINS of output frame o.  Unsigned 64-bit, floor division.  Candidate j is USED iff count_j >= max(1, L / 16); then a_j,c >= count_j > 0.
//       r_j,c = clamp((2 * 32768 * b_j,c + a_j,c) / (2 * a_j,c), 16384, 65536)                    (the fill blend's rounded Q15 ratio; terms < 2^63)
//       G_c   = (2 * (32768 + sum_j r_j,c) + (1 + m)) / (2 * (1 + m))        over the m used candidates
//     G_c is the rounded mean of the window's exposures relative to frame k, with k itself included as 32768.  (Statistics a caller made with
//     a_j,c == 0 under a used count lie outside what the statistics kernel can produce; r_j,c is 32768 there, so that nothing divides by zero.)
//   * APPLIED SAMPLE.  min((v * G_c + 16384) >> 15, max_value), unsigned 32-bit (65535 * 65536 + 16384 < 2^32).  A frame whose three gains are all
//     32768 is left as it is, bit for bit, samples above the maximum included.
//   * HENCE (a) n_cand == 1, a list that ends at once, candidates that lie outside the frame and candidates with fewer than max(1, L / 16)
//     counted pairs give the frame back bit for bit; (b) identical frames under identity maps come back bit for bit; (c) constant frames of 100
//     (target) and 200 (one candidate) give r = 65536, G = 49152 and every sample 150; (d) 16384 <= G_c <= 65536 whatever the content and the
//     maps; (e) a candidate that is the target under an integer shift with every sample halved exactly gives r_j = 16384.
//
// KERNELS.
// vs_k_exposure_stats: one launch over all (output frame, candidate j >= 1) pairs of a call, grid z = pair; the pair's entry (matrix, frame
// pointers: vsk::FillCand, 64 bytes) is read with scalar loads.  A wave owns 8 lattice rows x 256 lattice columns, in four column chunks of its 64
// lanes.  The position's sum starts with M0 x + M1 y, so what a row shares is the product M1 y (and M4 y), not M1 y + M2: lane r evaluates the
// two products of the strip's row r once and the wave reads them back with v_readlane (uniform values, the denoise kernel's arrangement); a lane
// evaluates M0 x, M3 x once per chunk.  Per lattice pixel: two fp64 additions per coordinate as the rule writes them (the file is compiled
// without contraction), rint, the range test, six sample loads, the six level tests, seven lane accumulators.  BOUND: a lane takes at most
// 8 * 4 = 32 pairs, so its sums stay below 32 * 65535 < 2^21 and a wave's below 2^27: uint32 accumulators, flushed once, at the end of the
// wave's fixed tile.  The wave reduces with cross-lane shuffles and lane 0 adds each non-zero share to the pair's uint64 with one atomicAdd (the
// channel-sums kernel's pattern).  The launcher zeroes the statistics on the same stream first.  No LDS, no barrier.
// vs_k_exposure_gains: one thread per output frame, the 64-bit divisions of the rule.
// vs_k_bgr_gain: the point-wise pass.  X4: a lane owns the 12 bytes of four (u8) or two (u16) consecutive pixels as three dwords (every row of
// source and destination on a dword); the pixels behind a row's last whole group, and every pixel of the other variant, go sample by sample: the
// same bytes.  The frame's three gains are scalar loads, clamped to 16384 .. 65536.  A frame with unit gains is skipped when its destination is
// its source and copied otherwise (unit gain is the identity of the arithmetic; only the saturation is lifted).  Every sample is read and
// written by the same lane, so in-place use is defined.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int ES_ROWS = 8, ES_CHUNKS = 4, ES_WAVES = 4;    // statistics: a wave's strip is 8 lattice rows x (4 x 64) lattice columns
constexpr int GN_ROWS = 16, GN_WAVES = 4;                  // gain pass: a wave owns 16 rows of its 64 lanes' pixel groups

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every gather, atomic and store of this file, sites 545-553: 545 / 546 the target's
// row and column offsets, 547 / 548 the candidate's, 549 the statistics word; 550 the gains kernel's reads, 551 its stores; 552 the gain pass's
// dword accesses (source and destination extents), 553 its per-sample ones.  The extents are written inside the macros' arguments.

// neither black nor clipped at 8-bit precision
__device__ __forceinline__ bool es_level_ok(uint32_t v, int shift) { return ((v >> shift) - 1u) < 254u; }

// cands: n_cand entries per output frame; entry 0 = the target, a null frame ends the list.  stats: 8 words per entry (zeroed by the launcher).
// blockIdx.z = pair: output frame z / (n_cand - 1), candidate 1 + z % (n_cand - 1).  lw x lh: the lattice.
template <typename T>
__global__ __launch_bounds__(64 * ES_WAVES) void vs_k_exposure_stats(const vsk::FillCand* __restrict__ cands, int n_cand, int w, int h, int src_stride,
                                                                     int shift, int step, int lw, int lh, unsigned long long* __restrict__ stats,
                                                                     int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int ly0 = (tyi * ES_WAVES + wv) * ES_ROWS, lx0 = txi * 64 * ES_CHUNKS;
    if (ly0 >= lh) return;                                                // wave-uniform
    const int o = (int)blockIdx.z / (n_cand - 1), j = 1 + (int)blockIdx.z - o * (n_cand - 1);
    cands += (size_t)o * (size_t)n_cand;
    // (the entries of a list are filled up to its end and null behind it: candidate j is in the list iff it has a frame)
    const GPtr<T> cs = (GPtr<T>)cands[j].src;
    if (!cs) return;                                                      // uniform
    const GPtr<T> tgt = (GPtr<T>)cands[0].src;
    const double M0 = cands[j].m[0], M1 = cands[j].m[1], M2 = cands[j].m[2], M3 = cands[j].m[3], M4 = cands[j].m[4], M5 = cands[j].m[5];
    const double yl = (double)(min(ly0 + (lane & (ES_ROWS - 1)), lh - 1) * step);       // the row whose products this lane evaluates
    const double m1yl = M1 * yl, m4yl = M4 * yl;
    const double wmax = (double)(w - 1), hmax = (double)(h - 1);
    uint32_t cnt = 0, a[3] = {0u, 0u, 0u}, b[3] = {0u, 0u, 0u};          // a lane's 32 pairs: < 2^21
#pragma unroll 1
    for (int ch = 0; ch < ES_CHUNKS; ch++) {
        if (lx0 + ch * 64 >= lw) break;                                   // wave-uniform
        const int lx = lx0 + ch * 64 + lane;
        const bool lane_in = lx < lw;
        const int x = min(lx, lw - 1) * step;                             // (lanes past the row compute on its last lattice column and count nothing)
        const double m0x = M0 * (double)x, m3x = M3 * (double)x;
#pragma unroll
        for (int r = 0; r < ES_ROWS; r++) {
            if (ly0 + r >= lh) break;                                     // wave-uniform
            const int y = (ly0 + r) * step;
            const double fx = rint((m0x + readlane_f64(m1yl, r)) + M2);
            const double fy = rint((m3x + readlane_f64(m4yl, r)) + M5);
            if (lane_in && fx >= 0.0 && fx <= wmax && fy >= 0.0 && fy <= hmax) {         // (false for NaN and the infinities)
                const GPtr<T> tp = tgt + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 545) + VS_IDX((size_t)x * 3, 3LL * w - 2, 546);
                const GPtr<T> qp = cs + VS_IDX((size_t)(int)fy * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 547) + VS_IDX((size_t)(int)fx * 3, 3LL * w - 2, 548);
                const uint32_t p0 = tp[0], p1 = tp[1], p2 = tp[2], q0 = qp[0], q1 = qp[1], q2 = qp[2];
                if (es_level_ok(p0, shift) && es_level_ok(p1, shift) && es_level_ok(p2, shift) && es_level_ok(q0, shift) && es_level_ok(q1, shift) &&
                    es_level_ok(q2, shift)) {
                    cnt++;
                    a[0] += p0; a[1] += p1; a[2] += p2;
                    b[0] += q0; b[1] += q1; b[2] += q2;
                }
            }
        }
    }
    unsigned long long* const out = stats + ((size_t)o * (size_t)n_cand + (size_t)j) * 8;
    const uint32_t v[7] = {cnt, a[0], a[1], a[2], b[0], b[1], b[2]};
#pragma unroll
    for (int k = 0; k < 7; k++) {                                         // a wave's share is below 2^27
        uint32_t sum = v[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0 && sum != 0) atomicAdd(out + VS_IDX(k, 8, 549), (unsigned long long)sum);
    }
}

// the rounded Q15 ratio b / a, clamped to [1/2, 2]
__device__ __forceinline__ unsigned long long ratio_q15(unsigned long long a, unsigned long long b) {
    const unsigned long long d = 2ull * a;                                // (0 for a == 0, and for a caller's a == 2^63)
    if (d == 0) return 32768ull;
    const unsigned long long g = (2ull * 32768ull * b + a) / d;
    return min(max(g, 16384ull), 65536ull);
}

// gains[4 o + {0..2: G_B, G_G, G_R, 3: m}] from stats[(o n_cand + j) 8 + ..]; thr = max(1, L / 16)
__global__ __launch_bounds__(64) void vs_k_exposure_gains(const unsigned long long* __restrict__ stats, int n_cand, int n_out, unsigned long long thr,
                                                          uint32_t* __restrict__ gains) {
    const int o = (int)(blockIdx.x * 64 + threadIdx.x);
    if (o >= n_out) return;
    const long long words = (long long)n_out * n_cand * 8;
    (void)words;
    unsigned long long sum[3] = {32768ull, 32768ull, 32768ull}, m = 0;
    for (int j = 1; j < n_cand; j++) {
        const size_t e = ((size_t)o * (size_t)n_cand + (size_t)j) * 8;
        if (stats[VS_IDX(e, words, 550)] < thr) continue;
        m++;
#pragma unroll
        for (int c = 0; c < 3; c++) sum[c] += ratio_q15(stats[VS_IDX(e + 1 + c, words, 550)], stats[VS_IDX(e + 4 + c, words, 550)]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) gains[VS_IDX(4 * (size_t)o + c, 4LL * n_out, 551)] = (uint32_t)((2ull * sum[c] + (1ull + m)) / (2ull * (1ull + m)));
    gains[VS_IDX(4 * (size_t)o + 3, 4LL * n_out, 551)] = (uint32_t)m;
}

__device__ __forceinline__ uint32_t gn_apply(uint32_t v, uint32_t g, uint32_t lim) { return min((v * g + 16384u) >> 15, lim); }

// frame blockIdx.y of src scaled by gains[4 blockIdx.y ..] into dst (dst may be src: no restrict)
template <typename T, bool X4>
__global__ __launch_bounds__(64 * GN_WAVES) void vs_k_bgr_gain(const T* src, int w, int h, int src_stride, size_t src_fs, const uint32_t* __restrict__ gains,
                                                               int maxv, T* dst, int dst_stride, size_t dst_fs, int tiles_x) {
    constexpr int G = X4 ? 12 / (3 * (int)sizeof(T)) : 1;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int y0 = (tyi * GN_WAVES + wv) * GN_ROWS;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + GN_ROWS, h);
    const int x = (txi * 64 + lane) * G;                                  // this lane's first pixel
    const T* const sf = src + (size_t)blockIdx.y * src_fs;
    T* const df = dst + (size_t)blockIdx.y * dst_fs;
    uint32_t g[3];                                                        // scalar loads
#pragma unroll
    for (int c = 0; c < 3; c++) g[c] = min(max(gains[4 * (size_t)blockIdx.y + c], 16384u), 65536u);
    const bool unit = g[0] == 32768u && g[1] == 32768u && g[2] == 32768u;
    if (unit && (const T*)df == sf) return;                               // uniform: nothing to do in place
    const uint32_t lim = unit ? 65535u : (uint32_t)maxv;                  // (unit gain is the identity; a copy does not saturate)
    const long long sext = (long long)(h - 1) * src_stride + 3LL * w, dext = (long long)(h - 1) * dst_stride + 3LL * w;   // elements of a frame
    (void)sext; (void)dext;
    for (int y = y0; y < y1; y++) {
        const size_t so = (size_t)y * (size_t)src_stride + (size_t)x * 3, dofs = (size_t)y * (size_t)dst_stride + (size_t)x * 3;
        if (X4 && x + G <= w) {
            const uint32_t* const q = (const uint32_t*)(sf + VS_IDX(so, sext - (3 * G - 1), 552));
            uint32_t* const op = (uint32_t*)(df + VS_IDX(dofs, dext - (3 * G - 1), 552));
            const uint32_t d[3] = {q[0], q[1], q[2]};
            uint32_t e[3] = {0u, 0u, 0u};
            if (sizeof(T) == 1) {
#pragma unroll
                for (int k = 0; k < 12; k++) px_put<T>(e, k, gn_apply(px_get<T>(d, k), g[k % 3], lim));
            } else {
#pragma unroll
                for (int k = 0; k < 6; k++) px_put<T>(e, k, gn_apply(px_get<T>(d, k), g[k % 3], lim));
            }
            op[0] = e[0]; op[1] = e[1]; op[2] = e[2];
        } else {
#pragma unroll
            for (int i = 0; i < G; i++)
                if (x + i < w) {
                    const T* const sp = sf + VS_IDX(so + 3 * i, sext - 2, 553);
                    T* const dp = df + VS_IDX(dofs + 3 * i, dext - 2, 553);
                    const uint32_t v0 = sp[0], v1 = sp[1], v2 = sp[2];
                    dp[0] = (T)gn_apply(v0, g[0], lim); dp[1] = (T)gn_apply(v1, g[1], lim); dp[2] = (T)gn_apply(v2, g[2], lim);
                }
        }
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_deflicker)

namespace vsk {

size_t exposure_threshold(int w, int h, int step) {
    const size_t L = (size_t)((w + step - 1) / step) * (size_t)((h + step - 1) / step);
    return std::max<size_t>(1, L / 16);
}

hipError_t exposure_stats(const FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int shift_to_8, int step, unsigned long long* stats,
                          int n_frames, hipStream_t s) {
    if ((bits != 8 && bits != 16) || shift_to_8 < 0 || shift_to_8 > 8 || n_cand < 1 || n_cand > 16 || n_frames < 1 || w < 1 || h < 1 || w > 32767 || h > 32767)
        return hipErrorNotSupported;
    if (step < 1 || step > 64) return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(stats, 0, (size_t)n_frames * (size_t)n_cand * 8 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    if (n_cand < 2) return hipSuccess;                                    // only the frames themselves: nothing to measure
    const int lw = (w + step - 1) / step, lh = (h + step - 1) / step;
    const int tiles_x = (lw + 64 * ES_CHUNKS - 1) / (64 * ES_CHUNKS), tiles_y = (lh + ES_ROWS * ES_WAVES - 1) / (ES_ROWS * ES_WAVES);
    const int per = 65535 / (n_cand - 1);                                 // gridDim.z limit: whole output frames per launch
    for (int f0 = 0; f0 < n_frames; f0 += per) {
        const int nf = std::min(n_frames - f0, per);
        const dim3 grid((unsigned)(tiles_x * tiles_y), 1u, (unsigned)(nf * (n_cand - 1))), block(64 * ES_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * (size_t)n_cand;
        unsigned long long* sp = stats + (size_t)f0 * (size_t)n_cand * 8;
        if (bits == 16)
            hipLaunchKernelGGL(vs_k_exposure_stats<uint16_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, shift_to_8, step, lw, lh, sp, tiles_x);
        else
            hipLaunchKernelGGL(vs_k_exposure_stats<uint8_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, shift_to_8, step, lw, lh, sp, tiles_x);
    }
    return hipGetLastError();
}

hipError_t exposure_gains(const unsigned long long* stats, int n_out, int n_cand, int w, int h, int step, uint32_t* gains, hipStream_t s) {
    if (n_out < 1 || n_cand < 1 || n_cand > 16 || w < 1 || h < 1 || step < 1 || step > 64) return hipErrorNotSupported;
    hipLaunchKernelGGL(vs_k_exposure_gains, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, s, stats, n_cand, n_out,
                       (unsigned long long)exposure_threshold(w, h, step), gains);
    return hipGetLastError();
}

hipError_t bgr_gain(const void* src, int w, int h, int src_stride, int bits, int max_value, const uint32_t* gains, void* dst, int dst_stride, int n_frames,
                    size_t src_fs, size_t dst_fs, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (w < 1 || h < 1 || n_frames < 1) return hipErrorNotSupported;
    const size_t esz = (size_t)bits / 8;
    // dword accesses where every row of every frame starts on a dword, in the source and in the destination
    const bool x4 = rows_on_dwords(src, src_stride, src_fs, n_frames, esz) && rows_on_dwords(dst, dst_stride, dst_fs, n_frames, esz);
    const int g = x4 ? (bits == 16 ? 2 : 4) : 1;
    const int tiles_x = (w + 64 * g - 1) / (64 * g), tiles_y = (h + GN_ROWS * GN_WAVES - 1) / (GN_ROWS * GN_WAVES);
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * GN_WAVES);
        const char* sp = (const char*)src + (size_t)f0 * src_fs * esz;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        const uint32_t* gp = gains + (size_t)f0 * 4;
        if (x4 && bits == 16)
            hipLaunchKernelGGL((vs_k_bgr_gain<uint16_t, true>), grid, block, 0, s, (const uint16_t*)sp, w, h, src_stride, src_fs, gp, max_value, (uint16_t*)dp, dst_stride, dst_fs, tiles_x);
        else if (x4)
            hipLaunchKernelGGL((vs_k_bgr_gain<uint8_t, true>), grid, block, 0, s, (const uint8_t*)sp, w, h, src_stride, src_fs, gp, max_value, (uint8_t*)dp, dst_stride, dst_fs, tiles_x);
        else if (bits == 16)
            hipLaunchKernelGGL((vs_k_bgr_gain<uint16_t, false>), grid, block, 0, s, (const uint16_t*)sp, w, h, src_stride, src_fs, gp, max_value, (uint16_t*)dp, dst_stride, dst_fs, tiles_x);
        else
            hipLaunchKernelGGL((vs_k_bgr_gain<uint8_t, false>), grid, block, 0, s, (const uint8_t*)sp, w, h, src_stride, src_fs, gp, max_value, (uint8_t*)dp, dst_stride, dst_fs, tiles_x);
    });
    return hipGetLastError();
}

}  // namespace vsk
