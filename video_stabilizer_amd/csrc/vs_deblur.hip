// vs_deblur.hip -- deblurring by transfer: the pixels of a frame that camera shake has blurred are blended with the pixels its SHARPER
// neighbours show at the same scene point (Matsushita et al. 2006; the role of OpenCV videostab's WeightingDeblurer).  The stabilizer feeds it
// the input frames that FOLLOW the output frame: they are already held in device memory and their motions are already measured.
//
// THE RULE (also include/vs_amd.h, vs_bgr_sharpness_batch / vs_bgr_deblur_batch; DESIGN.md "Deblur").  Interleaved BGR, every VS_FMT_BGR*.
//   * GRAY.  g = min(((B*3735 + G*19235 + R*9798 + 16384) >> 15) >> (bits - 8), 255): vs_bgr_to_gray's rule shifted to 8 bits.
//   * SHARPNESS of a frame: S = sum over 1 <= x <= w-2, 1 <= y <= h-2 of (g(x+1,y) - g(x-1,y))^2 + (g(x,y+1) - g(x,y-1))^2, a uint64_t (0 for
//     frames narrower or lower than 3).  Integer sums: exact whatever the order of the reduction.  S <= 130050 w h < 2^53, so (double)S is exact.
//   * CANDIDATES.  Output frame o has n_cand (1 .. 16) candidates (frame, transform t); candidate 0 is the target frame k itself (its
//     transform is ignored); a candidate without a frame ends the list.  Candidate j TAKES PART iff S_j > S_k, strictly, and then has
//     r_j = (float)min((double)S_j / (double)max(S_k, 1), (double)max_ratio).  If no candidate takes part the frame is copied.
//   * PER PIXEL.  With M = vs_cv_inverse_matrix(t_j) target pixel (x, y) lies in candidate j at qx = rint((M0 x + M1 y) + M2),
//     qy = rint((M3 x + M4 y) + M5): doubles, that order, no fma, ties to even -- VS_WARP_BILINEAR_CV's convention and centre.  Nearest
//     sample (interpolation is a blur).  Outside the frame the candidate contributes nothing at that pixel.  Otherwise, with
//     d = |g_k(x,y) - g_j(qx,qy)| as float, w = (r_j * r_j) / (d + sensitivity) in fp32 (correctly rounded division); per channel
//     acc_c = p_c + sum_j w q_c and W = 1 + sum_j w, summed in candidate order in fp32 without fma; out_c = floor(acc_c / W + 0.5)
//     saturated to the format's maximum.
//   * HENCE a frame with no sharper candidate, identical frames (ties on S) and n_cand == 1 all give the target back bit for bit.
//
// KERNELS.  vs_k_bgr_sharpness: a wave owns 62 columns x 32 rows of interior pixels; a lane computes the gray of its column once per row,
// takes the horizontal neighbours from the lanes beside it (lanes 0 and 63 are halo) and keeps the rows above and below in registers; one
// 64-bit vector atomic per wave merges the partial sum (the sums are integers: the order cannot matter).  vs_k_bgr_sharpness_x4 is the same
// walk with four pixels per lane and dword loads, for frames whose width and alignment allow it (the engine's dense frames do).  vs_k_deblur_ratio: one thread per
// output frame turns S_k, S_j into r_j^2 per candidate (-1: takes no part) -- the host never sees a sharpness.  vs_k_bgr_deblur: a wave owns
// 64 columns x 16 rows; which candidates take part is uniform over the frame, so the candidate loop is wave-uniform and the matrices and
// ratios are scalar loads; a tile of a frame with no sharper candidate is copied with dword accesses where the rows allow it.
// vs_k_bgr_deblur_x4 is the same pass with four pixels per lane, the target read and the result stored as dwords, for frames whose width and
// alignment allow it (the engine's dense frames do).  No LDS, no scratch, no barrier.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int SH_COLS = 62, SH_ROWS = 32, SH_WAVES = 4;   // sharpness: interior columns / rows per wave, waves (stacked) per workgroup
constexpr int DB_W = 64, DB_ROWS = 16, DB_WAVES = 4;      // deblur: a wave's strip, four strips stacked = a 64 x 64 tile

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every gather and every store of this file, sites 501-516: an element offset within
// a frame, the access's last sample included, lies below (h - 1) * stride + 3 w, source and destination alike (a pixel's address: its row offset
// at most (h - 1) * stride and its column offset, last sample included, below 3 w).  The extents are written inside
// the macros' arguments, which the regular build drops: its kernels are instruction for instruction what they were.

template <typename T>
__device__ __forceinline__ int gray8(const T* __restrict__ p, int shift) {
    const uint32_t g = (((uint32_t)p[0] * 3735u + (uint32_t)p[1] * 19235u + (uint32_t)p[2] * 9798u + 16384u) >> 15) >> shift;
    return (int)min(g, 255u);
}

// out[frame] (zeroed by the launcher on the same stream) += this wave's share of S
template <typename T>
__global__ __launch_bounds__(64 * SH_WAVES) void vs_k_bgr_sharpness(const T* __restrict__ src, int w, int h, int src_stride, int shift, size_t src_fs,
                                                                    unsigned long long* __restrict__ out, int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int ya = 1 + (tyi * SH_WAVES + wv) * SH_ROWS;                   // first interior row of this wave
    if (ya > h - 2) return;                                               // wave-uniform
    const int yb = min(ya + SH_ROWS, h - 1);                              // one past its last interior row
    const int x = txi * SH_COLS + lane;                                   // lanes 1 .. 62 own interior columns, 0 and 63 are their neighbours
    const bool centre = lane >= 1 && lane <= SH_COLS && x <= w - 2;
    const T* const col = src + (size_t)blockIdx.y * src_fs + (size_t)min(x, w - 1) * 3;
    int gu = gray8(col + VS_IDX((size_t)(ya - 1) * (size_t)src_stride, (long long)(h - 1) * src_stride + 3LL * w - 3LL * min(x, w - 1) - 2, 501), shift);
    int gm = gray8(col + VS_IDX((size_t)ya * (size_t)src_stride, (long long)(h - 1) * src_stride + 3LL * w - 3LL * min(x, w - 1) - 2, 501), shift);
    uint32_t acc = 0;                                                     // <= 32 * 130050
#pragma unroll 8
    for (int r = 0; r < SH_ROWS; r++) {                                   // (a fixed trip count: rows past the last one are read clamped and not counted)
        const int y = ya + r;
        const int gd = gray8(col + VS_IDX((size_t)min(y + 1, h - 1) * (size_t)src_stride, (long long)(h - 1) * src_stride + 3LL * w - 3LL * min(x, w - 1) - 2, 502), shift);
        const int dx = __shfl_down(gm, 1) - __shfl_up(gm, 1), dy = gd - gu;
        if (centre && y < yb) acc += (uint32_t)(dx * dx + dy * dy);
        gu = gm; gm = gd;
    }
    unsigned long long sum = acc;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0 && sum != 0) atomicAdd(out + blockIdx.y, sum);
}

// The same sum for frames whose rows allow dword loads (w a multiple of 4; frames, rows and frame stride 4-byte aligned): a lane owns FOUR
// consecutive pixels, read as three (u8) or six (u16) dwords, and keeps their grays packed in one register per row; a wave spans 256 pixels
// and counts those that have both horizontal neighbours in it (pixels 1 .. 252 of its span: the spans advance by 252).  One memory
// instruction per 4 (u8) / 2 (u16) bytes of a lane instead of one per sample: the byte-load version spent its time issuing loads.
constexpr int SV_COLS = 252;
template <typename T>
__device__ __forceinline__ uint32_t gray8x4(const uint32_t* __restrict__ p, int shift) {
    uint32_t s[12];
    if (sizeof(T) == 1) {
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
#pragma unroll
        for (int k = 0; k < 4; k++) { s[k] = (d0 >> (8 * k)) & 255u; s[4 + k] = (d1 >> (8 * k)) & 255u; s[8 + k] = (d2 >> (8 * k)) & 255u; }
    } else {
#pragma unroll
        for (int k = 0; k < 6; k++) { const uint32_t d = p[k]; s[2 * k] = d & 65535u; s[2 * k + 1] = d >> 16; }
    }
    uint32_t g = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t v = ((s[3 * i] * 3735u + s[3 * i + 1] * 19235u + s[3 * i + 2] * 9798u + 16384u) >> 15) >> shift;
        g |= min(v, 255u) << (8 * i);
    }
    return g;
}
template <typename T>
__global__ __launch_bounds__(64 * SH_WAVES) void vs_k_bgr_sharpness_x4(const T* __restrict__ src, int w, int h, int src_stride, int shift, size_t src_fs,
                                                                       unsigned long long* __restrict__ out, int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int ya = 1 + (tyi * SH_WAVES + wv) * SH_ROWS;
    if (ya > h - 2) return;                                               // wave-uniform
    const int yb = min(ya + SH_ROWS, h - 1);
    const int xs = txi * SV_COLS + 4 * lane;                              // this lane's first pixel; past the row: reads the row's last group, counts nothing
    const int x = min(xs, w - 4);
    uint32_t count = 0;                                                   // bit i: pixel i of the group is an interior pixel this wave counts
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int pi = 4 * lane + i;
        if (xs < w && pi >= 1 && pi <= SV_COLS && xs + i >= 1 && xs + i <= w - 2) count |= 1u << i;
    }
    const T* const col = src + (size_t)blockIdx.y * src_fs + (size_t)x * 3;
    // (twelve samples per read)
    uint32_t gu = gray8x4<T>((const uint32_t*)(col + VS_IDX((size_t)(ya - 1) * (size_t)src_stride, (long long)(h - 1) * src_stride + 3LL * w - 3LL * x - 11, 503)), shift);
    uint32_t gm = gray8x4<T>((const uint32_t*)(col + VS_IDX((size_t)ya * (size_t)src_stride, (long long)(h - 1) * src_stride + 3LL * w - 3LL * x - 11, 503)), shift);
    uint32_t acc = 0;                                                     // <= 4 * 32 * 130050
#pragma unroll 4
    for (int r = 0; r < SH_ROWS; r++) {
        const int y = ya + r;
        const uint32_t gd = gray8x4<T>((const uint32_t*)(col + VS_IDX((size_t)min(y + 1, h - 1) * (size_t)src_stride, (long long)(h - 1) * src_stride + 3LL * w - 3LL * x - 11, 504)), shift);
        const uint32_t left = __shfl_up(gm, 1) >> 24, right = __shfl_down(gm, 1) & 255u;
        const uint32_t live = y < yb ? count : 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int l = (int)(i ? (gm >> (8 * i - 8)) & 255u : left), rr = (int)(i < 3 ? (gm >> (8 * i + 8)) & 255u : right);
            const int dx = rr - l, dy = (int)((gd >> (8 * i)) & 255u) - (int)((gu >> (8 * i)) & 255u);
            if ((live >> i) & 1u) acc += (uint32_t)(dx * dx + dy * dy);
        }
        gu = gm; gm = gd;
    }
    unsigned long long sum = acc;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0 && sum != 0) atomicAdd(out + blockIdx.y, sum);
}

// r2[o * n_cand + c] = r_c^2 of output frame o's candidate c, or -1 when it takes no part (c == 0, S_c <= S_k, behind the end of the list)
__global__ __launch_bounds__(64) void vs_k_deblur_ratio(const vsk::DeblurCand* __restrict__ cands, int n_cand, int n_out, float max_ratio,
                                                        float* __restrict__ r2) {
    const int o = (int)(blockIdx.x * 64 + threadIdx.x);
    if (o >= n_out) return;
    cands += (size_t)o * (size_t)n_cand;
    r2 += (size_t)o * (size_t)n_cand;
    const unsigned long long sk = *cands[0].sharp;
    r2[0] = -1.0f;
    bool live = true;
    for (int c = 1; c < n_cand; c++) {
        live = live && cands[c].src != nullptr;
        float v = -1.0f;
        if (live) {
            const unsigned long long sj = *cands[c].sharp;
            if (sj > sk) {
                const float r = (float)fmin((double)sj / (double)max(sk, 1ull), (double)max_ratio);
                v = r * r;
            }
        }
        r2[c] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(64 * DB_WAVES) void vs_k_bgr_deblur(const vsk::DeblurCand* __restrict__ cands, const float* __restrict__ r2s, int n_cand, int w,
                                                                 int h, int src_stride, int shift, int maxv, float sens, T* __restrict__ dst,
                                                                 int dst_stride, size_t dst_fs, int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x0 = txi * DB_W, y0 = (tyi * DB_WAVES + wv) * DB_ROWS;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + DB_ROWS, h), nx = min(DB_W, w - x0);
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    r2s += (size_t)blockIdx.y * (size_t)n_cand;
    dst += (size_t)blockIdx.y * dst_fs;
    const T* const tgt = (const T*)cands[0].src;
    bool any = false;                                                     // uniform: the ratios are the same for every wave of the frame
    for (int c = 1; c < n_cand; c++) any = any || r2s[c] >= 0.0f;
    if (!any) {
        // no sharper candidate: a copy.  Rows whose both ends allow it move as dwords (the strip's first byte is 192 * sizeof(T) * txi into its row).
        // vs_cv_sample.hpp's strip_copy, written out: called from here it changes what the compiler makes of the candidate loop below
        // (profiles/lookahead_shared_sampler.md)
        const size_t row_bytes = (size_t)nx * 3 * sizeof(T);
        const bool wide = (((uintptr_t)tgt | (uintptr_t)dst | ((size_t)src_stride * sizeof(T)) | ((size_t)dst_stride * sizeof(T))) & 3) == 0;
        for (int y = y0; y < y1; y++) {
            const uint8_t* const sp = (const uint8_t*)(tgt + (size_t)y * (size_t)src_stride + (size_t)x0 * 3);
            uint8_t* const dp = (uint8_t*)(dst + (size_t)y * (size_t)dst_stride + (size_t)x0 * 3);
            size_t done = 0;
            if (wide) {
                const size_t nd = row_bytes / 4;
                for (size_t i = lane; i < nd; i += 64)
                    ((uint32_t*)dp)[VS_IDX(i, ((long long)(h - 1) * dst_stride + 3LL * w - ((long long)y * dst_stride + 3LL * x0)) * (long long)sizeof(T) / 4, 505)] = ((const uint32_t*)sp)[VS_IDX(i, ((long long)(h - 1) * src_stride + 3LL * w - ((long long)y * src_stride + 3LL * x0)) * (long long)sizeof(T) / 4, 506)];
                done = nd * 4;
            }
            for (size_t i = done + lane; i < row_bytes; i += 64)
                dp[VS_IDX(i, ((long long)(h - 1) * dst_stride + 3LL * w - ((long long)y * dst_stride + 3LL * x0)) * (long long)sizeof(T), 507)] = sp[VS_IDX(i, ((long long)(h - 1) * src_stride + 3LL * w - ((long long)y * src_stride + 3LL * x0)) * (long long)sizeof(T), 508)];
        }
        return;
    }
    const int x = x0 + lane;
    if (lane >= nx) return;                                               // (no cross-lane operation below)
    const double dxx = (double)x;
#pragma unroll 1
    for (int y = y0; y < y1; y++) {
        const double dyy = (double)y;
        const T* const tp = tgt + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 509) + VS_IDX((size_t)x * 3, 3LL * w - 2, 509);
        const int gk = gray8(tp, shift);
        float a0 = (float)tp[0], a1 = (float)tp[1], a2 = (float)tp[2], W = 1.0f;
#pragma unroll 1
        for (int c = 1; c < n_cand; c++) {                                // wave-uniform: ratio, matrix and frame pointer are scalar loads
            const float r2 = r2s[c];
            if (!(r2 >= 0.0f)) continue;
            const T* const cs = (const T*)cands[c].src;
            const double fx = rint((cands[c].m[0] * dxx + cands[c].m[1] * dyy) + cands[c].m[2]);
            const double fy = rint((cands[c].m[3] * dxx + cands[c].m[4] * dyy) + cands[c].m[5]);
            if (fx >= 0.0 && fx <= (double)(w - 1) && fy >= 0.0 && fy <= (double)(h - 1)) {       // (false for NaN)
                const T* const qp = cs + VS_IDX((size_t)(int)fy * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 510) + VS_IDX((size_t)(int)fx * 3, 3LL * w - 2, 510);
                const float q0 = (float)qp[0], q1 = (float)qp[1], q2 = (float)qp[2];
                const float d = fabsf((float)(gk - gray8(qp, shift)));
                const float wt = r2 / (d + sens);
                a0 = a0 + wt * q0; a1 = a1 + wt * q1; a2 = a2 + wt * q2;
                W = W + wt;
            }
        }
        T* const op = dst + VS_IDX((size_t)y * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 511) + VS_IDX((size_t)x * 3, 3LL * w - 2, 511);
        op[0] = (T)min(max((int)floorf(a0 / W + 0.5f), 0), maxv);
        op[1] = (T)min(max((int)floorf(a1 / W + 0.5f), 0), maxv);
        op[2] = (T)min(max((int)floorf(a2 / W + 0.5f), 0), maxv);
    }
}

// The same pass for frames whose rows allow dword accesses on the target and the destination (w a multiple of 4; target frames, destination,
// rows and frame strides 4-byte aligned): a lane owns four consecutive pixels, reads them as three (u8) or six (u16) dwords and stores them
// likewise; the gathers stay per sample (a candidate's pixel lies anywhere).  The arithmetic per pixel is the kernel's above, operation for
// operation.  A wave owns 256 columns x 16 rows.
template <typename T>
__global__ __launch_bounds__(64 * DB_WAVES) void vs_k_bgr_deblur_x4(const vsk::DeblurCand* __restrict__ cands, const float* __restrict__ r2s, int n_cand,
                                                                    int w, int h, int src_stride, int shift, int maxv, float sens, T* __restrict__ dst,
                                                                    int dst_stride, size_t dst_fs, int tiles_x) {
    constexpr int ND = 3 * (int)sizeof(T);                                // dwords of a lane's four pixels
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x0 = txi * 4 * DB_W, y0 = (tyi * DB_WAVES + wv) * DB_ROWS;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + DB_ROWS, h), nx = min(4 * DB_W, w - x0);
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    r2s += (size_t)blockIdx.y * (size_t)n_cand;
    dst += (size_t)blockIdx.y * dst_fs;
    const T* const tgt = (const T*)cands[0].src;
    bool any = false;                                                     // uniform
    for (int c = 1; c < n_cand; c++) any = any || r2s[c] >= 0.0f;
    if (!any) {                                                           // no sharper candidate: a copy, in dwords
        const size_t nd = (size_t)nx * 3 * sizeof(T) / 4;
        for (int y = y0; y < y1; y++) {
            const uint32_t* const sp = (const uint32_t*)(tgt + (size_t)y * (size_t)src_stride + (size_t)x0 * 3);
            uint32_t* const dp = (uint32_t*)(dst + (size_t)y * (size_t)dst_stride + (size_t)x0 * 3);
            for (size_t i = lane; i < nd; i += 64)
                dp[VS_IDX(i, ((long long)(h - 1) * dst_stride + 3LL * w - ((long long)y * dst_stride + 3LL * x0)) * (long long)sizeof(T) / 4, 512)] = sp[VS_IDX(i, ((long long)(h - 1) * src_stride + 3LL * w - ((long long)y * src_stride + 3LL * x0)) * (long long)sizeof(T) / 4, 513)];
        }
        return;
    }
    const int x = x0 + 4 * lane;
    if (x >= w) return;                                                   // (no cross-lane operation below)
#pragma unroll 1
    for (int y = y0; y < y1; y++) {
        const double dyy = (double)y;
        const uint32_t* const tp = (const uint32_t*)(tgt + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 514) + VS_IDX((size_t)x * 3, 3LL * w - 11, 514));      // (twelve samples)
        uint32_t d[ND];
#pragma unroll
        for (int k = 0; k < ND; k++) d[k] = tp[k];
        float a[12], W[4];
        int gk[4];
#pragma unroll
        for (int k = 0; k < 12; k++) a[k] = (float)px_get<T>(d, k);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t g = (((uint32_t)a[3 * i] * 3735u + (uint32_t)a[3 * i + 1] * 19235u + (uint32_t)a[3 * i + 2] * 9798u + 16384u) >> 15) >> shift;
            gk[i] = (int)min(g, 255u);
            W[i] = 1.0f;
        }
#pragma unroll 1
        for (int c = 1; c < n_cand; c++) {                                // wave-uniform
            const float r2 = r2s[c];
            if (!(r2 >= 0.0f)) continue;
            const T* const cs = (const T*)cands[c].src;
            const double m0 = cands[c].m[0], m1 = cands[c].m[1], m2 = cands[c].m[2], m3 = cands[c].m[3], m4 = cands[c].m[4], m5 = cands[c].m[5];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const double dxx = (double)(x + i);
                const double fx = rint((m0 * dxx + m1 * dyy) + m2);
                const double fy = rint((m3 * dxx + m4 * dyy) + m5);
                if (fx >= 0.0 && fx <= (double)(w - 1) && fy >= 0.0 && fy <= (double)(h - 1)) {       // (false for NaN)
                    const T* const qp = cs + VS_IDX((size_t)(int)fy * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 515) + VS_IDX((size_t)(int)fx * 3, 3LL * w - 2, 515);
                    const float q0 = (float)qp[0], q1 = (float)qp[1], q2 = (float)qp[2];
                    const float dg = fabsf((float)(gk[i] - gray8(qp, shift)));
                    const float wt = r2 / (dg + sens);
                    a[3 * i] = a[3 * i] + wt * q0; a[3 * i + 1] = a[3 * i + 1] + wt * q1; a[3 * i + 2] = a[3 * i + 2] + wt * q2;
                    W[i] = W[i] + wt;
                }
            }
        }
        uint32_t o[ND];
#pragma unroll
        for (int k = 0; k < ND; k++) o[k] = 0;
#pragma unroll
        for (int k = 0; k < 12; k++) {
            const uint32_t v = (uint32_t)min(max((int)floorf(a[k] / W[k / 3] + 0.5f), 0), maxv);
            px_put<T>(o, k, v);
        }
        uint32_t* const op = (uint32_t*)(dst + VS_IDX((size_t)y * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 516) + VS_IDX((size_t)x * 3, 3LL * w - 11, 516));
#pragma unroll
        for (int k = 0; k < ND; k++) op[k] = o[k];
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_deblur)

namespace vsk {

hipError_t bgr_sharpness(const void* src, int w, int h, int src_stride, int bits, int shift_to_8, unsigned long long* out, int n_frames, size_t src_fs,
                         hipStream_t s) {
    if ((bits != 8 && bits != 16) || shift_to_8 < 0 || shift_to_8 > 8 || n_frames < 1) return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_frames * sizeof(unsigned long long), s);
    if (e != hipSuccess || w < 3 || h < 3) return e;
    const size_t esz = (size_t)bits / 8;
    const bool x4 = w % 4 == 0 && rows_on_dwords(src, src_stride, src_fs, n_frames, esz);
    const int cols = x4 ? SV_COLS : SH_COLS;
    const int tiles_x = (w - 2 + cols - 1) / cols, tiles_y = (h - 2 + SH_ROWS * SH_WAVES - 1) / (SH_ROWS * SH_WAVES);
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * SH_WAVES);
        const char* sp = (const char*)src + (size_t)f0 * src_fs * esz;
        if (x4 && bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_sharpness_x4<uint16_t>, grid, block, 0, s, (const uint16_t*)sp, w, h, src_stride, shift_to_8, src_fs, out + f0, tiles_x);
        else if (x4)
            hipLaunchKernelGGL(vs_k_bgr_sharpness_x4<uint8_t>, grid, block, 0, s, (const uint8_t*)sp, w, h, src_stride, shift_to_8, src_fs, out + f0, tiles_x);
        else if (bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_sharpness<uint16_t>, grid, block, 0, s, (const uint16_t*)sp, w, h, src_stride, shift_to_8, src_fs, out + f0, tiles_x);
        else
            hipLaunchKernelGGL(vs_k_bgr_sharpness<uint8_t>, grid, block, 0, s, (const uint8_t*)sp, w, h, src_stride, shift_to_8, src_fs, out + f0, tiles_x);
    });
    return hipGetLastError();
}

hipError_t bgr_deblur(const DeblurCand* cands_dev, float* r2_dev, int n_cand, int w, int h, int src_stride, int bits, int shift_to_8, int max_value,
                      float sensitivity, float max_ratio, void* dst, int dst_stride, int n_frames, size_t dst_fs, bool targets_aligned, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (shift_to_8 < 0 || shift_to_8 > 8 || n_cand < 1 || n_frames < 1 || w < 1 || h < 1) return hipErrorNotSupported;
    hipLaunchKernelGGL(vs_k_deblur_ratio, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, s, cands_dev, n_cand, n_frames, max_ratio, r2_dev);
    const size_t esz = (size_t)bits / 8;
    // four pixels per lane with dword accesses where every target row and every destination row starts on a dword
    const bool x4 = targets_aligned && w % 4 == 0 && rows_on_dwords(nullptr, src_stride, 0, 1, esz) && rows_on_dwords(dst, dst_stride, dst_fs, n_frames, esz);
    const int tw = x4 ? 4 * DB_W : DB_W;
    const int tiles_x = (w + tw - 1) / tw, tiles_y = (h + DB_ROWS * DB_WAVES - 1) / (DB_ROWS * DB_WAVES);
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * DB_WAVES);
        const DeblurCand* cp = cands_dev + (size_t)f0 * (size_t)n_cand;
        const float* rp = r2_dev + (size_t)f0 * (size_t)n_cand;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        if (x4 && bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_deblur_x4<uint16_t>, grid, block, 0, s, cp, rp, n_cand, w, h, src_stride, shift_to_8, max_value, sensitivity, (uint16_t*)dp,
                               dst_stride, dst_fs, tiles_x);
        else if (x4)
            hipLaunchKernelGGL(vs_k_bgr_deblur_x4<uint8_t>, grid, block, 0, s, cp, rp, n_cand, w, h, src_stride, shift_to_8, max_value, sensitivity, (uint8_t*)dp,
                               dst_stride, dst_fs, tiles_x);
        else if (bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_deblur<uint16_t>, grid, block, 0, s, cp, rp, n_cand, w, h, src_stride, shift_to_8, max_value, sensitivity, (uint16_t*)dp,
                               dst_stride, dst_fs, tiles_x);
        else
            hipLaunchKernelGGL(vs_k_bgr_deblur<uint8_t>, grid, block, 0, s, cp, rp, n_cand, w, h, src_stride, shift_to_8, max_value, sensitivity, (uint8_t*)dp,
                               dst_stride, dst_fs, tiles_x);
    });
    return hipGetLastError();
}

}  // namespace vsk
