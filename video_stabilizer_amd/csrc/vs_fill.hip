// vs_fill.hip -- border fill for VS_WARP_BILINEAR_CV: the pixels of a warped frame that its own source does not cover are taken from other
// source frames (the stabilizer: the input frames that FOLLOW the output frame, already held in device memory).
//
// THE RULE (also include/vs_amd.h, vs_bgr_image_warp_fill_batch; DESIGN.md "Border fill").  3 channels, 8-bit or 16-bit containers, both
// borders, frames up to 32767 x 32767.  An output frame has n_cand >= 1 candidates, each a (source frame, forward transform t) pair in
// VS_WARP_BILINEAR_CV's convention: t is what cv::warpAffine is handed, M = vs_cv_inverse_matrix(t) is the output -> source matrix.
// Candidate 0 is the frame itself.
//   * For a candidate, output pixel (x, y) -- full-frame coordinates, also under a ROI -- has the integer source position of the existing warp:
//       X = (X0[y] + adelta[x]) >> 5,  sx = X >> 5        X0[y] = cvRound((M[1] y + M[2]) 1024) + 16,  adelta[x] = cvRound(M[0] x 1024)
//       Y = (Y0[y] + bdelta[x]) >> 5,  sy = Y >> 5        Y0[y] = cvRound((M[4] y + M[5]) 1024) + 16,  bdelta[x] = cvRound(M[3] x 1024)
//     All of it in int32 as in cv::warpAffine: cvRound saturates to [INT_MIN, INT_MAX] (NaN -> 0; cv_round_sat), the additions (+ 16 in
//     cv_row_origin, X0 + adelta in cv_pos) wrap in two's complement, the shifts are arithmetic.  An extreme matrix is judged on the saturated,
//     wrapped position: the one pass 1 samples.
//     The candidate COVERS the pixel iff all four taps lie in the frame: 0 <= sx && sx + 1 <= w - 1 && 0 <= sy && sy + 1 <= h - 1.
//   * The pixel's value is the value VS_WARP_BILINEAR_CV gives for the FIRST candidate that covers it, bit for bit (8-bit: integer weights,
//     (sum + 512) >> 10; 16-bit: float weights a b / 1024, cvRound, saturated to max_value).  A candidate without a frame ends the list.  If
//     no candidate covers the pixel it keeps candidate 0's ordinary result under `border`.
//   * Hence the pixels candidate 0 covers are exactly the plain warp's output, and n_cand == 1 IS the plain warp.  No blending, no
//     feathering, no photometric matching here: those are the two switches of THE BLEND RULE below (vs_k_bgr_warp_cv_fill_blend_c3), off by
//     default; with both off this kernel serves the call as it always did.
//
// TWO PASSES.  Pass 1 is the existing warp launch for candidate 0 (vs_warp.hip, untouched).  Pass 2 is the kernel below, on the same stream,
// over the output of all frames of the run.  X(x, y) is a term monotone in x plus a term monotone in y, so a rectangle of output pixels is
// covered by candidate 0 iff its four corner pixels are (eight table terms, uniform values).  A workgroup owns a 256 x 256 block: it tests the
// block and leaves when it is covered -- all but the blocks on the frame's rim; otherwise its four waves walk the block's 64 x 16 strips and
// test each strip the same way.  (One workgroup per 64 x 64 tile with the strip test alone was measured first: 1.7 us per 4K frame
// when nothing is uncovered -- 8160 waves that start, test and leave -- against 0.5 us with the block test; DESIGN.md section 14 has both
// versions' figures, also for the rim work, which that version spread over more waves.)  In the remaining strips a lane whose pixel candidate 0 covers stores nothing;
// the others walk the candidates in a wave-uniform loop (the matrices are scalar loads), evaluate cvRound in double per pixel as
// cv::warpAffine does per table entry, gather the four taps straight from global memory and store.  A covered pixel has all four taps
// inside the frame, so no border rule is applied here and a store never goes to a pixel pass 1 got right.  No LDS, no barrier.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_cover.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

// (the strip and block constants FL_* and cv_covers_rect: vs_cover.hpp, shared with the coverage index of vs_inpaint.hip)

// one output pixel of a candidate that covers it, all four taps inside the frame: vs_cv_sample.hpp's cv_sample_inside on the first tap
template <typename T>
__device__ __forceinline__ void fill_sample(const T* __restrict__ src, int stride, CvPos p, int maxv, T* __restrict__ out) {
    uint32_t q[3];
    cv_sample_inside<T>(src + (size_t)(p.Y >> 5) * (size_t)stride + (size_t)(p.X >> 5) * 3, stride, p, maxv, q);
    out[0] = (T)q[0]; out[1] = (T)q[1]; out[2] = (T)q[2];
}

// cands: n_cand entries per output frame (gridDim.y frames); entry 0 = the frame itself (its matrix only), a null frame ends the list
template <typename T>
__global__ __launch_bounds__(64 * FL_WAVES) void vs_k_bgr_warp_cv_fill_c3(const vsk::FillCand* __restrict__ cands, int n_cand, int w, int h, int src_stride,
                                                                        int maxv, T* __restrict__ dst, int dst_stride, size_t dst_fs, vsk::Roi roi,
                                                                        int blocks_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int byi = (int)blockIdx.x / blocks_x, bxi = (int)blockIdx.x - byi * blocks_x;
    const int bx0 = bxi * FL_BLOCK, by0 = byi * FL_BLOCK;                  // this workgroup's block in the output window
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    dst += (size_t)blockIdx.y * dst_fs;
    double M[6];
#pragma unroll
    for (int k = 0; k < 6; k++) M[k] = cands[0].m[k];
    if (cv_covers_rect(M, roi, bx0, by0, min(FL_BLOCK, roi.w - bx0), min(FL_BLOCK, roi.h - by0), w, h)) return;       // uniform
#pragma unroll 1
    for (int t = 0; t < (FL_BLOCK / FL_W) * (FL_BLOCK / (FL_ROWS * FL_WAVES)); t++) {
        const int x0 = bx0 + (t % (FL_BLOCK / FL_W)) * FL_W, y0 = by0 + ((t / (FL_BLOCK / FL_W)) * FL_WAVES + wv) * FL_ROWS;     // this wave's strip
        if (x0 >= roi.w || y0 >= roi.h) continue;                          // wave-uniform
        const int nx = min(FL_W, roi.w - x0), ny = min(FL_ROWS, roi.h - y0);  // live columns / rows (>= 1)
        if (cv_covers_rect(M, roi, x0, y0, nx, ny, w, h)) continue;        // wave-uniform
        const int x = x0 + lane;
        const bool lane_in = lane < nx;
        const int fx = min(x, roi.w - 1) + roi.x;
        const int ad0 = cv_delta(M[0], fx), bd0 = cv_delta(M[3], fx);
#pragma unroll 1
        for (int r = 0; r < ny; r++) {
            const int y = y0 + r, fy = y + roi.y;
            bool open = lane_in && !cv_covers(cv_pos(cv_row_origin(M[1], M[2], fy), cv_row_origin(M[4], M[5], fy), ad0, bd0), w, h);
            T* const px = dst + (size_t)y * (size_t)dst_stride + (size_t)x * 3;
#pragma unroll 1
            for (int c = 1; c < n_cand; c++) {               // wave-uniform: the candidate's entry is read with scalar loads
                if (__builtin_amdgcn_ballot_w64(open) == 0) break;
                const T* const cs = (const T*)cands[c].src;
                if (!cs) break;
                double C[6];
#pragma unroll
                for (int k = 0; k < 6; k++) C[k] = cands[c].m[k];
                const CvPos p = cv_pos(cv_row_origin(C[1], C[2], fy), cv_row_origin(C[4], C[5], fy), cv_delta(C[0], fx), cv_delta(C[3], fx));
                if (open && cv_covers(p, w, h)) {
                    T o[3];
#ifdef VS_DEBUG_BOUNDS
                    // the bounds build (vs_device.hpp), sites 521 / 522: the 2 x 2 taps' last sample, at stride + 5 from the first, lies inside the source
                    // frame's (h - 1) * stride + 3 w elements -- else pixel (0, 0) is sampled; the store's last sample lies inside the output window
                    const bool taps_in = vsd::bounds_ok((long long)(p.Y >> 5) * src_stride + 3LL * (p.X >> 5) + src_stride + 5, (long long)(h - 1) * src_stride + 3LL * w, 521);
                    fill_sample(cs, src_stride, taps_in ? p : CvPos{0, 0}, maxv, o);
                    if (!vsd::bounds_ok((long long)y * dst_stride + 3LL * x + 2, (long long)(roi.h - 1) * dst_stride + 3LL * roi.w, 522)) continue;
#else
                    fill_sample(cs, src_stride, p, maxv, o);
#endif
                    px[0] = o[0]; px[1] = o[1]; px[2] = o[2];
                    open = false;
                }
            }
        }
    }
}


// ---- THE BLEND RULE (also include/vs_amd.h, vs_bgr_image_warp_fill_blend_batch; DESIGN.md "Fill blend") ----------------------------------
// Two independent switches on the fill, exact integer rules.  Candidates, coverage, the int32 positions X, Y (5 fraction bits) and the sample
// q_c of a covering candidate are the fill's above.
//   * CHANNEL SUMS.  S_i,c = the sum of the raw samples of channel c over all w x h pixels of frame i, uint64 (no clamp to the format's
//     maximum; <= 65535 * 32767^2 < 2^46; integers: the order of the reduction cannot matter).
//   * GAIN (match == 1) of candidate j >= 1 for output frame k (candidate 0's frame), per channel, Q15, unsigned 64-bit, floor division:
//       G = 32768                                                        if S_j,c == 0 or S_k,c == 0
//       G = clamp((2 * 32768 * S_k,c + S_j,c) / (2 * S_j,c), 16384, 65536)   otherwise          (every term < 2^63)
//     With match == 0, G = 32768.
//   * MATCHED FILL SAMPLE of the first candidate j >= 1 that covers the pixel: f_c = min((q_c * G + 16384) >> 15, max_value), unsigned 32-bit
//     (65535 * 65536 + 16384 < 2^32).  G = 32768 passes q_c through unchanged.
//   * UNCOVERED PIXEL (candidate 0 does not cover it): f_c if a later candidate covers it; else candidate 0's result under `border`, as ever.
//   * BAND PIXEL (feather >= 1): K = 32 << feather, Xmax = (w - 1) * 32 - 1, Ymax = (h - 1) * 32 - 1.  A pixel candidate 0 covers has
//     0 <= X <= Xmax, 0 <= Y <= Ymax; d = min(X, Xmax - X, Y, Ymax - Y), k = d + 1.  If k >= K or no later candidate covers the pixel it is the
//     plain warp's value p_c bit for bit; otherwise out_c = (k * p_c + (K - k) * f_c + K / 2) >> (5 + feather)  (< 2^27: unsigned 32-bit).
//   * Hence (a) feather == 0 && match == 0 is the fill above bit for bit; (b) n_cand == 1 or a list without a later candidate is the plain ROI
//     warp; (c) a band pixel lies between min(p_c, f_c) and max(p_c, f_c); (d) identical frames under identity maps come back bit for bit with
//     any setting; (e) a pixel at least 2^feather source pixels inside candidate 0's frame is never changed.
//
// PASSES.  Pass 1 is the warp launch for candidate 0, as in the fill.  With match on, vs_k_fill_gains (one thread per output frame) turns the two
// sum pointers of every candidate entry into three Q15 gains of 17 bits, packed into the entry's eight reserved bytes: the host never sees a
// sum.  Pass 2 is vs_k_bgr_warp_cv_fill_blend_c3, one launch over all frames of the run on the same stream: the fill kernel's block / strip walk with
// the test "candidate 0 covers the rectangle" replaced by "DEEP INSIDE": all four corner positions have d >= K - 1 (X is a term monotone in x plus
// a term monotone in y, so the corners bound the rectangle; the same 2^29 guard on the table terms).  A band lane reads pass 1's value back from
// dst (written on this stream before the launch) and blends; the gains are scalar loads, wave-uniform per candidate.  No LDS, no barrier.

constexpr int CS_ROWS = 16, CS_WAVES = 4;                  // channel sums: a wave sums 16 rows of its 64 lanes' pixel groups
constexpr unsigned long long kUnitGains = 32768ull | (32768ull << 17) | (32768ull << 34);

// out[3 * frame + c] (zeroed by the launcher on the same stream) += this wave's share of S_c.  X4: a lane owns the 12 bytes of four (u8) or two
// (u16) consecutive pixels and reads them as three dwords (every row starts on a dword); the pixels behind the row's last whole group, and every
// pixel of the other variant, are read sample by sample.
template <typename T, bool X4>
__global__ __launch_bounds__(64 * CS_WAVES) void vs_k_bgr_channel_sums(const T* __restrict__ src, int w, int h, int src_stride, size_t src_fs,
                                                                       unsigned long long* __restrict__ out, int tiles_x) {
    constexpr int G = X4 ? 12 / (3 * (int)sizeof(T)) : 1;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int y0 = (tyi * CS_WAVES + wv) * CS_ROWS;
    if (y0 >= h) return;                                                  // wave-uniform
    const int y1 = min(y0 + CS_ROWS, h);
    const int x = (txi * 64 + lane) * G;                                  // this lane's first pixel
    const T* const frame = src + (size_t)blockIdx.y * src_fs;
    const long long extent = (long long)(h - 1) * src_stride + 3LL * w;   // elements of a frame
    (void)extent;
    uint32_t a[3] = {0u, 0u, 0u};                                         // <= 16 rows * 4 * 255 or 16 * 2 * 65535
    for (int y = y0; y < y1; y++) {
        const size_t ro = (size_t)y * (size_t)src_stride + (size_t)x * 3;
        if (X4 && x + G <= w) {
            const uint32_t* const q = (const uint32_t*)(frame + VS_IDX(ro, extent - (3 * G - 1), 526));
            const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
            if (sizeof(T) == 1) {                                          // B G R B | G R B G | R B G R
                a[0] += (d0 & 255u) + (d0 >> 24) + ((d1 >> 16) & 255u) + ((d2 >> 8) & 255u);
                a[1] += ((d0 >> 8) & 255u) + (d1 & 255u) + (d1 >> 24) + ((d2 >> 16) & 255u);
                a[2] += ((d0 >> 16) & 255u) + ((d1 >> 8) & 255u) + (d2 & 255u) + (d2 >> 24);
            } else {                                                       // B G | R B | G R
                a[0] += (d0 & 65535u) + (d1 >> 16);
                a[1] += (d0 >> 16) + (d2 & 65535u);
                a[2] += (d1 & 65535u) + (d2 >> 16);
            }
        } else {
#pragma unroll
            for (int i = 0; i < G; i++)
                if (x + i < w) {
                    const T* const px = frame + VS_IDX(ro + 3 * i, extent - 2, 527);
                    a[0] += px[0]; a[1] += px[1]; a[2] += px[2];
                }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {                                          // a wave's share is below 2^32: 64 lanes * 2^21
        uint32_t sum = a[c];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0 && sum != 0) atomicAdd(out + 3 * (size_t)blockIdx.y + c, (unsigned long long)sum);
    }
}

// Q15 gain of a candidate with sums sj for an output frame with sums sk (the rule above)
__device__ __forceinline__ unsigned long long fill_gain_q15(unsigned long long sk, unsigned long long sj) {
    if (sk == 0 || sj == 0) return 32768ull;
    const unsigned long long g = (2ull * 32768ull * sk + sj) / (2ull * sj);
    return min(max(g, 16384ull), 65536ull);
}
// every candidate entry c >= 1 of output frame o arrives with reserved = where its frame's three sums lie, entry 0 with where the output frame's
// lie; the entries c >= 1 leave with their three gains packed (17 bits each)
__global__ __launch_bounds__(64) void vs_k_fill_gains(vsk::FillCand* __restrict__ cands, int n_cand, int n_out) {
    const int o = (int)(blockIdx.x * 64 + threadIdx.x);
    if (o >= n_out) return;
    cands += (size_t)o * (size_t)n_cand;
    const unsigned long long* const sk = (const unsigned long long*)(uintptr_t)cands[0].reserved;
    for (int c = 1; c < n_cand; c++) {
        if (!cands[c].src) break;
        const unsigned long long* const sj = (const unsigned long long*)(uintptr_t)cands[c].reserved;
        cands[c].reserved = fill_gain_q15(sk[0], sj[0]) | (fill_gain_q15(sk[1], sj[1]) << 17) | (fill_gain_q15(sk[2], sj[2]) << 34);
    }
}

// candidate 0 (matrix M) has d >= m at every pixel of the nx x ny rectangle at (x0, y0) of the output window; m == 0: it covers every pixel
// (cv_covers_rect: X >= 0 and X <= Xmax is sx >= 0 and sx + 1 <= w - 1).  Same guard on the table terms.
__device__ __forceinline__ bool cv_deep_rect(const double M[6], vsk::Roi roi, int x0, int y0, int nx, int ny, int w, int h, int m) {
    const int fxA = x0 + roi.x, fxB = x0 + nx - 1 + roi.x, fyA = y0 + roi.y, fyB = y0 + ny - 1 + roi.y;
    const int adA = cv_delta(M[0], fxA), adB = cv_delta(M[0], fxB), bdA = cv_delta(M[3], fxA), bdB = cv_delta(M[3], fxB);
    const int XA = cv_row_origin(M[1], M[2], fyA), XB = cv_row_origin(M[1], M[2], fyB);
    const int YA = cv_row_origin(M[4], M[5], fyA), YB = cv_row_origin(M[4], M[5], fyB);
    const int lim = 1 << 29;
    const int lo = min(min(min(adA, adB), min(bdA, bdB)), min(min(XA, XB), min(YA, YB)));
    const int hi = max(max(max(adA, adB), max(bdA, bdB)), max(max(XA, XB), max(YA, YB)));
    const bool small = lo > -lim && hi < lim;
    const int mnX = min(XA, XB) + min(adA, adB), mxX = max(XA, XB) + max(adA, adB);
    const int mnY = min(YA, YB) + min(bdA, bdB), mxY = max(YA, YB) + max(bdA, bdB);
    const int Xmax = (w - 1) * 32 - 1, Ymax = (h - 1) * 32 - 1;
    return small && (mnX >> 5) >= m && (mxX >> 5) <= Xmax - m && (mnY >> 5) >= m && (mxY >> 5) <= Ymax - m;
}

template <typename T>
__global__ __launch_bounds__(64 * FL_WAVES) void vs_k_bgr_warp_cv_fill_blend_c3(const vsk::FillCand* __restrict__ cands, int n_cand, int w, int h,
                                                                              int src_stride, int maxv, int feather, T* __restrict__ dst,
                                                                              int dst_stride, size_t dst_fs, vsk::Roi roi, int blocks_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int byi = (int)blockIdx.x / blocks_x, bxi = (int)blockIdx.x - byi * blocks_x;
    const int bx0 = bxi * FL_BLOCK, by0 = byi * FL_BLOCK;
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    dst += (size_t)blockIdx.y * dst_fs;
    const int K = 32 << feather, margin = feather > 0 ? K - 1 : 0;         // feather == 0: K = 32 = k of every covered pixel, no band
    const int Xmax = (w - 1) * 32 - 1, Ymax = (h - 1) * 32 - 1;
    double M[6];
#pragma unroll
    for (int k = 0; k < 6; k++) M[k] = cands[0].m[k];
    if (cv_deep_rect(M, roi, bx0, by0, min(FL_BLOCK, roi.w - bx0), min(FL_BLOCK, roi.h - by0), w, h, margin)) return;       // uniform
#pragma unroll 1
    for (int t = 0; t < (FL_BLOCK / FL_W) * (FL_BLOCK / (FL_ROWS * FL_WAVES)); t++) {
        const int x0 = bx0 + (t % (FL_BLOCK / FL_W)) * FL_W, y0 = by0 + ((t / (FL_BLOCK / FL_W)) * FL_WAVES + wv) * FL_ROWS;     // this wave's strip
        if (x0 >= roi.w || y0 >= roi.h) continue;                          // wave-uniform
        const int nx = min(FL_W, roi.w - x0), ny = min(FL_ROWS, roi.h - y0);
        if (cv_deep_rect(M, roi, x0, y0, nx, ny, w, h, margin)) continue;  // wave-uniform
        const int x = x0 + lane;
        const bool lane_in = lane < nx;
        const int fx = min(x, roi.w - 1) + roi.x;
        const int ad0 = cv_delta(M[0], fx), bd0 = cv_delta(M[3], fx);
#pragma unroll 1
        for (int r = 0; r < ny; r++) {
            const int y = y0 + r, fy = y + roi.y;
            const CvPos p0 = cv_pos(cv_row_origin(M[1], M[2], fy), cv_row_origin(M[4], M[5], fy), ad0, bd0);
            const bool cov0 = cv_covers(p0, w, h);
            // the plain value's weight k of a pixel candidate 0 covers (K: outside the band)
            const int kk = cov0 && feather > 0 ? min(min(min(p0.X, Xmax - p0.X), min(p0.Y, Ymax - p0.Y)) + 1, K) : K;
            bool open = lane_in && (!cov0 || kk < K);
            T* const px = dst + (size_t)y * (size_t)dst_stride + (size_t)x * 3;
#pragma unroll 1
            for (int c = 1; c < n_cand; c++) {               // wave-uniform: the candidate's entry is read with scalar loads
                if (__builtin_amdgcn_ballot_w64(open) == 0) break;
                const T* const cs = (const T*)cands[c].src;
                if (!cs) break;
                double C[6];
#pragma unroll
                for (int k = 0; k < 6; k++) C[k] = cands[c].m[k];
                const unsigned long long gains = cands[c].reserved;
                const CvPos p = cv_pos(cv_row_origin(C[1], C[2], fy), cv_row_origin(C[4], C[5], fy), cv_delta(C[0], fx), cv_delta(C[3], fx));
                if (open && cv_covers(p, w, h)) {
                    T q[3];
#ifdef VS_DEBUG_BOUNDS
                    // the bounds build (vs_device.hpp), sites 523 / 524 / 525: the taps as in the fill kernel; the read-back and the store's last
                    // sample lie inside the output window
                    const bool taps_in = vsd::bounds_ok((long long)(p.Y >> 5) * src_stride + 3LL * (p.X >> 5) + src_stride + 5, (long long)(h - 1) * src_stride + 3LL * w, 523);
                    fill_sample(cs, src_stride, taps_in ? p : CvPos{0, 0}, maxv, q);
                    if (!vsd::bounds_ok((long long)y * dst_stride + 3LL * x + 2, (long long)(roi.h - 1) * dst_stride + 3LL * roi.w, cov0 ? 524 : 525)) continue;
#else
                    fill_sample(cs, src_stride, p, maxv, q);
#endif
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) {
                        const uint32_t G = (uint32_t)(gains >> (17 * ch)) & 0x1ffffu;
                        uint32_t f = min(((uint32_t)q[ch] * G + 16384u) >> 15, (uint32_t)maxv);
                        if (cov0) f = ((uint32_t)kk * (uint32_t)px[ch] + (uint32_t)(K - kk) * f + (uint32_t)(K >> 1)) >> (5 + feather);
                        q[ch] = (T)f;
                    }
                    px[0] = q[0]; px[1] = q[1]; px[2] = q[2];
                    open = false;
                }
            }
        }
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_fill)

namespace vsk {

hipError_t bgr_warp_cv_fill_c3(const FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int max_value, void* dst, int dst_stride,
                               int n_frames, size_t dst_fs, Roi roi, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (w > 32767 || h > 32767 || n_cand < 1) return hipErrorNotSupported;
    const int blocks_x = (roi.w + FL_BLOCK - 1) / FL_BLOCK, blocks_y = (roi.h + FL_BLOCK - 1) / FL_BLOCK;
    const size_t esz = (size_t)bits / 8;
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)nf), block(64 * FL_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * (size_t)n_cand;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        if (bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_warp_cv_fill_c3<uint16_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, max_value, (uint16_t*)dp, dst_stride, dst_fs, roi, blocks_x);
        else
            hipLaunchKernelGGL(vs_k_bgr_warp_cv_fill_c3<uint8_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, max_value, (uint8_t*)dp, dst_stride, dst_fs, roi, blocks_x);
    });
    return hipGetLastError();
}

unsigned long long fill_unit_gains() { return kUnitGains; }

hipError_t bgr_channel_sums(const void* src, int w, int h, int src_stride, int bits, unsigned long long* out, int n_frames, size_t src_fs, hipStream_t s) {
    if ((bits != 8 && bits != 16) || w < 1 || h < 1 || w > 32767 || h > 32767 || n_frames < 1) return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_frames * 3 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const size_t esz = (size_t)bits / 8;
    const bool x4 = rows_on_dwords(src, src_stride, src_fs, n_frames, esz);      // dword loads
    const int g = x4 ? (bits == 16 ? 2 : 4) : 1;
    const int tiles_x = (w + 64 * g - 1) / (64 * g), tiles_y = (h + CS_ROWS * CS_WAVES - 1) / (CS_ROWS * CS_WAVES);
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)nf), block(64 * CS_WAVES);
        const char* sp = (const char*)src + (size_t)f0 * src_fs * esz;
        unsigned long long* op = out + (size_t)f0 * 3;
        if (x4 && bits == 16)
            hipLaunchKernelGGL((vs_k_bgr_channel_sums<uint16_t, true>), grid, block, 0, s, (const uint16_t*)sp, w, h, src_stride, src_fs, op, tiles_x);
        else if (x4)
            hipLaunchKernelGGL((vs_k_bgr_channel_sums<uint8_t, true>), grid, block, 0, s, (const uint8_t*)sp, w, h, src_stride, src_fs, op, tiles_x);
        else if (bits == 16)
            hipLaunchKernelGGL((vs_k_bgr_channel_sums<uint16_t, false>), grid, block, 0, s, (const uint16_t*)sp, w, h, src_stride, src_fs, op, tiles_x);
        else
            hipLaunchKernelGGL((vs_k_bgr_channel_sums<uint8_t, false>), grid, block, 0, s, (const uint8_t*)sp, w, h, src_stride, src_fs, op, tiles_x);
    });
    return hipGetLastError();
}

hipError_t bgr_warp_cv_fill_blend_c3(FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int max_value, int feather, bool match, void* dst,
                                     int dst_stride, int n_frames, size_t dst_fs, Roi roi, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (w > 32767 || h > 32767 || n_cand < 1 || feather < 0 || feather > 6) return hipErrorNotSupported;
    if (match) hipLaunchKernelGGL(vs_k_fill_gains, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, s, cands_dev, n_cand, n_frames);
    const int blocks_x = (roi.w + FL_BLOCK - 1) / FL_BLOCK, blocks_y = (roi.h + FL_BLOCK - 1) / FL_BLOCK;
    const size_t esz = (size_t)bits / 8;
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)nf), block(64 * FL_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * (size_t)n_cand;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        if (bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_warp_cv_fill_blend_c3<uint16_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, max_value, feather, (uint16_t*)dp, dst_stride, dst_fs, roi, blocks_x);
        else
            hipLaunchKernelGGL(vs_k_bgr_warp_cv_fill_blend_c3<uint8_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, max_value, feather, (uint8_t*)dp, dst_stride, dst_fs, roi, blocks_x);
    });
    return hipGetLastError();
}

}  // namespace vsk
