// vs_scene.hip -- scene-cut detection: the frame difference of two consecutive frames taken THROUGH their measured motion.  The aligner is no cut
// detector: across a hard cut its Gauss-Newton loop often converges to some small similarity and reports success, and every look-ahead pass then
// borrows from the next scene.  The library holds both frames in device memory and has just measured the motion between them; inside a scene the
// difference through that motion is close to zero however hard the camera shakes, across a cut it is large whatever the aligner made of it.
//
// THE SCENE-CUT RULE (also include/vs_amd.h, vs_bgr_scene_stats_batch).
// Interleaved BGR, every VS_FMT_BGR*, frames up to 32767 a side; s = bits - 8.
//   - PARAMETERS.  step is 1 .. 64 (default 4, the deflicker's lattice); threshold is 1 .. 255, in 8-bit levels (default 32: above a 20 % exposure
//     jump and below every cut of the synthetic clips it was measured on -- a starting value, not a calibrated one).
//   - PAIR AND LATTICE.  A pair is (target frame, candidate frame, forward transform t in VS_WARP_BILINEAR_CV's convention): what a deflicker or
//     denoise candidate list gives for candidate 1.  The lattice pixels are those with x % step == 0 && y % step == 0;
//     L = ceil(w / step) * ceil(h / step).
//   - POSITION.  With M = vs_cv_inverse_matrix(t) lattice pixel (x, y) lies in the candidate at qx = rint((M0 x + M1 y) + M2),
//     qy = rint((M3 x + M4 y) + M5): doubles, that order, no fma, ties to even -- the deflicker's and deblur's nearest-sample position.  The
//     lattice pixel COUNTS iff qx, qy are finite, 0 <= qx <= w - 1 and 0 <= qy <= h - 1.  There is no level test: black and clipped samples count.
//   - STATISTIC.  With v' = min(v, max_value) >> s, each pair yields two uint64: count, and sad = the sum over the counted lattice pixels of
//     sum_c |p'_c - q'_c| (p the target at (x, y), q the candidate at (qx, qy)).  count < 2^30 and sad < 3 * 255 * 2^30; integer sums: the
//     order of the reduction cannot matter.  A NaN or infinite map counts nothing.
//   - DECISION.  Unsigned 64-bit: the pair is a CUT iff count < max(1, L / 16) or sad > 3 * threshold * count.  The inequality is strict:
//     equality is no cut.  Too little overlap is a cut: nothing shows that the frames are one scene, and nothing could be borrowed from the
//     candidate anyway.
//   - HENCE (a) identical frames under the identity give sad == 0; (b) a frame and its copy shifted by whole pixels, under that shift, give
//     sad == 0 and count = the overlap's lattice count; (c) constant frames of 100 and 130 give sad == 90 * count.
//
// KERNEL.
// vs_k_scene_stats: one launch over all pairs of a call, grid z = pair; the pair's two entries (target, then candidate with its matrix:
// vsk::FillCand, 64 bytes each) are read with scalar loads.  The shape is vs_k_exposure_stats' (vs_deflicker.hip): a wave owns 8 lattice rows x
// 256 lattice columns, in four column chunks of its 64 lanes; lane r evaluates the products M1 y and M4 y of the strip's row r once and the wave
// reads them back with v_readlane; a lane evaluates M0 x, M3 x once per chunk.  Per lattice pixel: two fp64 additions per coordinate as the rule
// writes them (the file is compiled without contraction), rint, the range test, six sample loads, three clamped shifts a side, three absolute
// differences, two lane accumulators.  BOUND: a lane takes at most 8 * 4 = 32 lattice pixels, so its count stays at 32 and its sad below
// 32 * 3 * 255 < 2^15; a wave's below 2^21: uint32 accumulators, flushed once, at the end of the wave's fixed tile.  The wave reduces with
// cross-lane shuffles and lane 0 adds each non-zero share to the pair's uint64 with one atomicAdd.  The launcher zeroes the statistics on the
// same stream first.  No LDS, no barrier.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int SC_ROWS = 8, SC_CHUNKS = 4, SC_WAVES = 4;    // a wave's strip is 8 lattice rows x (4 x 64) lattice columns

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every gather and atomic of this file, sites 616-620: 616 / 617 the target's row and
// column offsets, 618 / 619 the candidate's, 620 the statistics word.  The extents are written inside the macros' arguments.

// the sample at 8-bit precision: saturated to the format's maximum first
__device__ __forceinline__ int sc_level(uint32_t v, uint32_t maxv, int shift) { return (int)(min(v, maxv) >> shift); }

// cands: two entries per pair -- the target (its matrix is not read), the candidate with the output -> source matrix; a null frame on either side
// leaves the pair's statistics zero.  stats: 2 words per pair (zeroed by the launcher).  blockIdx.z = pair.  lw x lh: the lattice.
template <typename T>
__global__ __launch_bounds__(64 * SC_WAVES) void vs_k_scene_stats(const vsk::FillCand* __restrict__ cands, int w, int h, int src_stride, int shift,
                                                                  uint32_t maxv, int step, int lw, int lh, unsigned long long* __restrict__ stats,
                                                                  int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int ly0 = (tyi * SC_WAVES + wv) * SC_ROWS, lx0 = txi * 64 * SC_CHUNKS;
    if (ly0 >= lh) return;                                                // wave-uniform
    cands += (size_t)blockIdx.z * 2;
    const GPtr<T> tgt = (GPtr<T>)cands[0].src, cs = (GPtr<T>)cands[1].src;
    if (!tgt || !cs) return;                                              // uniform
    const double M0 = cands[1].m[0], M1 = cands[1].m[1], M2 = cands[1].m[2], M3 = cands[1].m[3], M4 = cands[1].m[4], M5 = cands[1].m[5];
    const double yl = (double)(min(ly0 + (lane & (SC_ROWS - 1)), lh - 1) * step);       // the row whose products this lane evaluates
    const double m1yl = M1 * yl, m4yl = M4 * yl;
    const double wmax = (double)(w - 1), hmax = (double)(h - 1);
    uint32_t cnt = 0, sad = 0;                                            // a lane's 32 lattice pixels: cnt <= 32, sad <= 32 * 3 * 255 < 2^15
#pragma unroll 1
    for (int ch = 0; ch < SC_CHUNKS; ch++) {
        if (lx0 + ch * 64 >= lw) break;                                   // wave-uniform
        const int lx = lx0 + ch * 64 + lane;
        const bool lane_in = lx < lw;
        const int x = min(lx, lw - 1) * step;                             // (lanes past the row compute on its last lattice column and count nothing)
        const double m0x = M0 * (double)x, m3x = M3 * (double)x;
#pragma unroll
        for (int r = 0; r < SC_ROWS; r++) {
            if (ly0 + r >= lh) break;                                     // wave-uniform
            const int y = (ly0 + r) * step;
            const double fx = rint((m0x + readlane_f64(m1yl, r)) + M2);
            const double fy = rint((m3x + readlane_f64(m4yl, r)) + M5);
            if (lane_in && fx >= 0.0 && fx <= wmax && fy >= 0.0 && fy <= hmax) {         // (false for NaN and the infinities)
                const GPtr<T> tp = tgt + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 616) + VS_IDX((size_t)x * 3, 3LL * w - 2, 617);
                const GPtr<T> qp = cs + VS_IDX((size_t)(int)fy * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 618) + VS_IDX((size_t)(int)fx * 3, 3LL * w - 2, 619);
                const uint32_t p0 = tp[0], p1 = tp[1], p2 = tp[2], q0 = qp[0], q1 = qp[1], q2 = qp[2];
                cnt++;
                sad += (uint32_t)abs(sc_level(p0, maxv, shift) - sc_level(q0, maxv, shift)) + (uint32_t)abs(sc_level(p1, maxv, shift) - sc_level(q1, maxv, shift)) +
                       (uint32_t)abs(sc_level(p2, maxv, shift) - sc_level(q2, maxv, shift));
            }
        }
    }
    unsigned long long* const out = stats + (size_t)blockIdx.z * 2;
    const uint32_t v[2] = {cnt, sad};
#pragma unroll
    for (int k = 0; k < 2; k++) {                                         // a wave's share is below 2^21
        uint32_t sum = v[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0 && sum != 0) atomicAdd(out + VS_IDX(k, 2, 620), (unsigned long long)sum);
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_scene)

namespace vsk {

hipError_t scene_stats(const FillCand* cands_dev, int w, int h, int src_stride, int bits, int shift_to_8, int max_value, int step, unsigned long long* stats,
                       int n_pairs, hipStream_t s) {
    if (!container_ok(bits, max_value) || shift_to_8 < 0 || shift_to_8 > 8 || n_pairs < 1 || w < 1 || h < 1 || w > 32767 || h > 32767 || src_stride < 3 * w)
        return hipErrorNotSupported;
    if (step < 1 || step > 64) return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(stats, 0, (size_t)n_pairs * 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const int lw = (w + step - 1) / step, lh = (h + step - 1) / step;
    const int tiles_x = (lw + 64 * SC_CHUNKS - 1) / (64 * SC_CHUNKS), tiles_y = (lh + SC_ROWS * SC_WAVES - 1) / (SC_ROWS * SC_WAVES);
    for_frame_chunks(n_pairs, [&](int f0, int nf) {                       // gridDim.z limit
        const dim3 grid((unsigned)(tiles_x * tiles_y), 1u, (unsigned)nf), block(64 * SC_WAVES);
        const FillCand* cp = cands_dev + (size_t)f0 * 2;
        unsigned long long* sp = stats + (size_t)f0 * 2;
        if (bits == 16)
            hipLaunchKernelGGL(vs_k_scene_stats<uint16_t>, grid, block, 0, s, cp, w, h, src_stride, shift_to_8, (uint32_t)max_value, step, lw, lh, sp, tiles_x);
        else
            hipLaunchKernelGGL(vs_k_scene_stats<uint8_t>, grid, block, 0, s, cp, w, h, src_stride, shift_to_8, (uint32_t)max_value, step, lw, lh, sp, tiles_x);
    });
    return hipGetLastError();
}

}  // namespace vsk
