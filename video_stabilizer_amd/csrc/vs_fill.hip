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
//     feathering, no photometric matching.
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

using namespace vsd;

namespace {

constexpr int FL_W = 64, FL_ROWS = 16, FL_WAVES = 4;      // a wave's strip: 64 columns x 16 rows; four strips stacked = a 64 x 64 tile
constexpr int FL_BLOCK = 256;                              // a workgroup's block of output pixels (a side): 4 x 4 tiles
static_assert(FL_BLOCK % FL_W == 0 && FL_BLOCK % (FL_ROWS * FL_WAVES) == 0, "whole tiles");

struct CvPos { int X, Y; };                                // 5 fraction bits each
__device__ __forceinline__ CvPos cv_pos(int X0, int Y0, int ad, int bd) {
    return CvPos{(int)((unsigned)X0 + (unsigned)ad) >> 5, (int)((unsigned)Y0 + (unsigned)bd) >> 5};
}
__device__ __forceinline__ bool cv_covers(CvPos p, int w, int h) {
    const int sx = p.X >> 5, sy = p.Y >> 5;
    return sx >= 0 && sx + 1 <= w - 1 && sy >= 0 && sy + 1 <= h - 1;
}

// candidate 0 (matrix M) covers every pixel of the nx x ny rectangle at (x0, y0) of the output window.  Every table term within 2^29: the sums
// cannot wrap, and with monotone terms the extremes of X and Y over the rectangle are sums of corner terms.
__device__ __forceinline__ bool cv_covers_rect(const double M[6], vsk::Roi roi, int x0, int y0, int nx, int ny, int w, int h) {
    const int fxA = x0 + roi.x, fxB = x0 + nx - 1 + roi.x, fyA = y0 + roi.y, fyB = y0 + ny - 1 + roi.y;
    const int adA = cv_delta(M[0], fxA), adB = cv_delta(M[0], fxB), bdA = cv_delta(M[3], fxA), bdB = cv_delta(M[3], fxB);
    const int XA = cv_row_origin(M[1], M[2], fyA), XB = cv_row_origin(M[1], M[2], fyB);
    const int YA = cv_row_origin(M[4], M[5], fyA), YB = cv_row_origin(M[4], M[5], fyB);
    const int lim = 1 << 29;
    // (-lim < term < lim asked of the terms as they stand: a delta that cvRound saturated to INT_MIN has no absolute value in int, and abs() would
    // hand it back negative -- "small".  Reached by a near-singular candidate 0 on a one-row window at frame row 0: tests/test_fill_hostile_gpu.py)
    const int lo = min(min(min(adA, adB), min(bdA, bdB)), min(min(XA, XB), min(YA, YB)));
    const int hi = max(max(max(adA, adB), max(bdA, bdB)), max(max(XA, XB), max(YA, YB)));
    const bool small = lo > -lim && hi < lim;
    const int mnX = min(XA, XB) + min(adA, adB), mxX = max(XA, XB) + max(adA, adB);
    const int mnY = min(YA, YB) + min(bdA, bdB), mxY = max(YA, YB) + max(bdA, bdB);
    // ((X0 + adelta) >> 5) >> 5 = (X0 + adelta) >> 10
    return small && (mnX >> 10) >= 0 && (mxX >> 10) + 1 <= w - 1 && (mnY >> 10) >= 0 && (mxY >> 10) + 1 <= h - 1;
}

// one output pixel of a candidate that covers it: all four taps inside the frame
__device__ __forceinline__ void cv_sample_inside(const uint8_t* __restrict__ src, int stride, CvPos p, int, uint8_t* __restrict__ out) {
    const int a1 = p.X & 31, b1 = p.Y & 31, a0 = 32 - a1, b0 = 32 - b1;
    const uint8_t* r0 = src + (size_t)(p.Y >> 5) * (size_t)stride + (size_t)(p.X >> 5) * 3;
    const uint8_t* r1 = r0 + stride;
#pragma unroll
    for (int c = 0; c < 3; c++)
        out[c] = (uint8_t)(((int)r0[c] * (a0 * b0) + (int)r0[c + 3] * (a1 * b0) + (int)r1[c] * (a0 * b1) + (int)r1[c + 3] * (a1 * b1) + 512) >> 10);
}
__device__ __forceinline__ void cv_sample_inside(const uint16_t* __restrict__ src, int stride, CvPos p, int maxv, uint16_t* __restrict__ out) {
    const int a1 = p.X & 31, b1 = p.Y & 31, a0 = 32 - a1, b0 = 32 - b1;
    const uint16_t* r0 = src + (size_t)(p.Y >> 5) * (size_t)stride + (size_t)(p.X >> 5) * 3;
    const uint16_t* r1 = r0 + stride;
    const float k = 1.0f / 1024.0f;
    const float w00 = (float)(a0 * b0) * k, w01 = (float)(a1 * b0) * k, w10 = (float)(a0 * b1) * k, w11 = (float)(a1 * b1) * k;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float sum = (float)r0[c] * w00 + (float)r0[c + 3] * w01 + (float)r1[c] * w10 + (float)r1[c + 3] * w11;
        out[c] = (uint16_t)min(max((int)rintf(sum), 0), maxv);
    }
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
                    cv_sample_inside(cs, src_stride, taps_in ? p : CvPos{0, 0}, maxv, o);
                    if (!vsd::bounds_ok((long long)y * dst_stride + 3LL * x + 2, (long long)(roi.h - 1) * dst_stride + 3LL * roi.w, 522)) continue;
#else
                    cv_sample_inside(cs, src_stride, p, maxv, o);
#endif
                    px[0] = o[0]; px[1] = o[1]; px[2] = o[2];
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
    if (bits == 16 ? (max_value < 0 || max_value > 65535) : (bits != 8 || max_value != 255)) return hipErrorNotSupported;
    if (w > 32767 || h > 32767 || n_cand < 1) return hipErrorNotSupported;
    const int blocks_x = (roi.w + FL_BLOCK - 1) / FL_BLOCK, blocks_y = (roi.h + FL_BLOCK - 1) / FL_BLOCK;
    const size_t esz = (size_t)bits / 8;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {         // gridDim.y limit
        const int nf = std::min(n_frames - f0, 65535);
        const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)nf), block(64 * FL_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * (size_t)n_cand;
        char* dp = (char*)dst + (size_t)f0 * dst_fs * esz;
        if (bits == 16)
            hipLaunchKernelGGL(vs_k_bgr_warp_cv_fill_c3<uint16_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, max_value, (uint16_t*)dp, dst_stride, dst_fs, roi, blocks_x);
        else
            hipLaunchKernelGGL(vs_k_bgr_warp_cv_fill_c3<uint8_t>, grid, block, 0, s, cp, n_cand, w, h, src_stride, max_value, (uint8_t*)dp, dst_stride, dst_fs, roi, blocks_x);
    }
    return hipGetLastError();
}

}  // namespace vsk
