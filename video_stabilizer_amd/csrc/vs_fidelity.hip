// vs_fidelity.hip -- fidelity statistics of image pairs: the squared error per channel and on gray, and an integer SSIM over 8 x 8 windows.  The
// passes that change output pixels (fill, blend, inpaint, deblur, denoise, deflicker, rolling shutter, lens, sharpen, scene cuts) are specified to
// the bit; what they do to the PICTURE had no measure.  The stabilization literature scores a clip by ITF, the mean PSNR between consecutive
// output frames; denoise and deblur work uses PSNR and SSIM against a reference clip.  Both frames already lie in device memory: one
// pass that reads each of them once gives every sum those scores need (what it costs, and what binds it: DESIGN.md section 29), and the scores themselves are a few divisions on the host (vs_fidelity_scores).
//
// THE FIDELITY RULE (also include/vs_amd.h, vs_bgr_fidelity_batch).
//   - SCOPE.  Interleaved BGR, every VS_FMT_BGR*, images of 1 .. 32767 pixels a side; s = bits - 8.  Every sample is first v' = min(v, max_value).
//   - PAIR.  A pair is (image a, image b), both w x h.  Each side has its own row stride and frame stride.  An image may be a window of a larger
//     frame: its origin pointer with the frame's strides.  Row starts may therefore fall on any byte (8-bit) or any element (16-bit).
//   - GRAY.  g = min(((B' * 3735 + G' * 19235 + R' * 9798 + 16384) >> 15) >> s, 255), unsigned 32-bit: vs_bgr_to_gray's weights.  The largest
//     value is 65535 * 32768 + 16384 < 2^32.
//   - WORDS.  Each pair gives six uint64: 0 .. 2 sse_b, sse_g, sse_r = the sum over all pixels of (a'_c - b'_c)^2, at the format's own precision;
//     3 sse_y = the same sum on g; 4 n_win; 5 ssim_sum, an int64 in two's complement.
//   - WINDOWS.  8 x 8 at a stride of 4: nwx = w >= 8 ? (w - 8) / 4 + 1 : 0, nwy likewise from h, n_win = nwx * nwy.  Window (i, j) covers x in
//     4i .. 4i + 7 and y in 4j .. 4j + 7.  Pixels right of, or below, the last window belong to no window; they still count in the four SSE words.
//   - PER WINDOW.  All on g, all in int32.  s1 = sum g_a, s2 = sum g_b, ss = sum (g_a^2 + g_b^2), s12 = sum g_a g_b;
//       vars = 64 ss - s1^2 - s2^2,  cov = 64 s12 - s1 s2;  c1 = 26634, c2 = 239708 ((0.01 * 255)^2 * 64^2 and (0.03 * 255)^2 * 64^2, rounded);
//       A = 2 s1 s2 + c1,  B = 2 cov + c2,  C = s1^2 + s2^2 + c1,  D = vars + c2;
//       q = rint(((double)(int64)(A * B) / (double)(int64)(C * D)) * 65536.0): the conversions and the division correctly rounded, no fma, ties
//       to even.  ssim_sum = sum q.
//   - BOUNDS.  s1, s2 <= 16320 and ss <= 8 323 200; each of vars, |cov|, A, |B|, C, D is at most 532 924 508 < 2^31 and the products stay below
//     2^59; C >= c1 and D >= c2, so both are positive; |q| <= 65536, because 2 s1 s2 <= s1^2 + s2^2 and 2 |cov| <= vars.
//     sse_c <= 65535^2 * 2^30 < 2^62, n_win < 2^26, |ssim_sum| < 2^42.
//   - HENCE (a) a == b gives zero SSE words and ssim_sum = 65536 * n_win; (b) 8-bit constant images of 100 and 130 give 900 w h in each SSE word
//     and q = 63344 in every window; (c) all-0 against all-maximum gives max_value^2 * w h per channel, 65025 w h for sse_y and q = 7; (d) an 8-bit
//     checkerboard of 0 / 255 against its inverse gives q = -65300; (e) exchanging a and b changes no word.
//   - Integer sums only: the order of the reduction cannot matter, so results are identical from run to run.
// The constants come from the usual SSIM derivation with population variances over 64 samples; they are this build's specification.  Values are
// close to, but not equal to, what other tools print: those scale c1 differently, weight the window with a Gaussian and finish in fp32.
//
// KERNEL.
// vs_k_fidelity: one launch over all pairs of a call, grid z = pair; the pair's entry (two image pointers, vsk::FidPair, 16 bytes) is read with
// scalar loads.  Both images are read once.  The picture is cut into 4 x 4 BLOCKS; window (i, j) is the four blocks (i, j), (i + 1, j),
// (i, j + 1), (i + 1, j + 1), so a window's four sums are sums of block sums.  A lane owns one block column and a wave walks a strip of 64 block
// columns downwards, a block row (four image rows) at a time: a lane adds its block's four sums to those of its block in the previous block
// row, takes its right neighbour's vertical pair with one cross-lane shuffle per sum, and has the window.
//   SEAMS.  Lane 63 has no right neighbour, so strips OVERLAP by one block column: a strip advances by FD_STRIP_PX = 4 * 63 pixels; lane 63
//   reads its block for the windows of lane 62 and adds nothing to the SSE words, and evaluates no window -- its block column is lane 0 of
//   the next strip, which does both.  A wave's band is FD_BAND_PX = 64 rows (16 block rows); a band that is not the first also reads the block row
//   ABOVE it, for the window row that straddles the seam, and adds nothing of that row to the SSE words.  So pixel (x, y) enters the SSE words in
//   strip (x / 4) / 63, band (y / 4) / 16 alone, and window (i, j) is evaluated in strip i / 63, band (j + 1) / 16 alone.  A workgroup is four
//   consecutive bands of one strip (FD_TILE_PX = 256 rows).
//   LOADS.  X4 (every row of both batches starts on a dword, vsk::rows_on_dwords): a lane's 4 pixels are 12 bytes = three dwords (8-bit) or 24
//   bytes = six dwords (16-bit); a row of the strip is 768 / 1536 consecutive bytes.  A block that the image's right edge cuts, and every block
//   of the other variant, is read sample by sample: the same values.
//   ACCUMULATORS.  A lane counts at most 16 block rows x 16 pixels = 256 pixels and 16 windows.  One squared 16-bit difference can already
//   exceed 2^31 (65535^2 = 4 294 836 225 < 2^32 fits an unsigned dword, two of them do not), so a 32-bit lane accumulator is wrong for 16-bit
//   containers from the second pixel on: sse_b, sse_g, sse_r are uint64 in the lane for 16-bit containers (256 * 65535^2 < 2^40; a wave's share
//   < 2^46) and uint32 for 8-bit ones (256 * 65025 < 2^24; a wave's < 2^30).  sse_y: uint32, as the 8-bit channels.  n_win: uint32, a lane's
//   <= 16, a wave's <= 1008.  ssim_sum: int32, a lane's |sum| <= 16 * 65536 = 2^20, a wave's < 2^26; it is sign-extended to 64 bits before the
//   atomic, which adds in two's complement.  The block sums: s1, s2 <= 16 * 255, ss <= 16 * 2 * 65025, s12 <= 16 * 65025, int32.
//   The wave reduces with cross-lane shuffles and lane 0 adds each non-zero share to the pair's uint64 with one atomicAdd.  The launcher zeroes
//   the statistics on the same stream first.  No LDS, no barrier.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int FD_COLS = 63, FD_BAND = 16, FD_WAVES = 4;    // a wave's strip: 63 owned block columns (+ lane 63's), 16 owned block rows (+ the one above)
constexpr int FD_STRIP_PX = 4 * FD_COLS, FD_BAND_PX = 4 * FD_BAND, FD_TILE_PX = FD_BAND_PX * FD_WAVES;      // 252, 64, 256: the seams of the tiling
constexpr int FD_C1 = 26634, FD_C2 = 239708;

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every load and atomic of this file, sites 629-636: 629 image a's row offset, 630 its
// dword column offset (a whole block: 12 elements), 631 its per-sample column offset; 632 / 633 / 634 the same of image b; 635 the statistics word;
// 636 the pair's entry.  The extents are written inside the macros' arguments.

typedef const VS_GLOBAL_AS uint32_t* fd_gdw;

// the lane accumulator of a channel's squared error: see ACCUMULATORS
template <typename T> struct FdAcc { typedef uint32_t type; };
template <> struct FdAcc<uint16_t> { typedef unsigned long long type; };

__device__ __forceinline__ uint32_t fd_gray(uint32_t b, uint32_t g, uint32_t r, int shift) {
    return min(((b * 3735u + g * 19235u + r * 9798u + 16384u) >> 15) >> shift, 255u);
}

// one row of a lane's block: npx pixels of image a (da) and image b (db), packed as they lie in memory
template <typename T>
__device__ __forceinline__ void fd_row(const uint32_t* da, const uint32_t* db, int npx, uint32_t maxv, int shift, bool counts,
                                       typename FdAcc<T>::type sse[3], uint32_t& sse_y, int blk[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (i < npx) {
            uint32_t pa[3], pb[3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                pa[c] = min(px_get<T>(da, 3 * i + c), maxv);
                pb[c] = min(px_get<T>(db, 3 * i + c), maxv);
            }
            const int ga = (int)fd_gray(pa[0], pa[1], pa[2], shift), gb = (int)fd_gray(pb[0], pb[1], pb[2], shift);
            if (counts) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const uint32_t d = pa[c] > pb[c] ? pa[c] - pb[c] : pb[c] - pa[c];
                    sse[c] += (typename FdAcc<T>::type)(d * d);          // (65535^2 < 2^32)
                }
                sse_y += (uint32_t)((ga - gb) * (ga - gb));
            }
            blk[0] += ga; blk[1] += gb; blk[2] += ga * ga + gb * gb; blk[3] += ga * gb;
        }
    }
}

// npx pixels at row + x0 * 3 into packed dwords.  dwords: the whole block with dword loads (X4 and the block is whole)
template <typename T, int SITE>
__device__ __forceinline__ void fd_load(GPtr<T> row, int x0, int npx, int w, bool dwords, uint32_t* d) {
    constexpr int ND = 3 * (int)sizeof(T);
    (void)w;
    if (dwords) {
        const fd_gdw q = (fd_gdw)(row + VS_IDX((size_t)x0 * 3, 3LL * w - 11, SITE));
#pragma unroll
        for (int k = 0; k < ND; k++) d[k] = q[k];
    } else {
#pragma unroll
        for (int k = 0; k < ND; k++) d[k] = 0u;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (i < npx) {
#pragma unroll
                for (int c = 0; c < 3; c++) px_put<T>(d, 3 * i + c, (uint32_t)row[VS_IDX((size_t)(x0 + i) * 3 + c, 3LL * w, SITE + 1)]);
            }
    }
}

// pairs: one entry per pair (blockIdx.z), image a and image b, both w x h; stats: 6 words per pair (zeroed by the launcher).  blockIdx.x = band group
// * strips + strip.
template <typename T, bool X4>
__global__ __launch_bounds__(64 * FD_WAVES) void vs_k_fidelity(const vsk::FidPair* __restrict__ pairs, int n_pairs, int w, int h, int a_stride, int b_stride,
                                                               int shift, uint32_t maxv, unsigned long long* __restrict__ stats, int strips) {
    constexpr int ND = 3 * (int)sizeof(T);
    typedef typename FdAcc<T>::type Acc;
    (void)n_pairs;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int bgi = (int)blockIdx.x / strips, strip = (int)blockIdx.x - bgi * strips;
    const int br0 = (bgi * FD_WAVES + wv) * FD_BAND;                      // the band's first own block row
    if (br0 * 4 >= h) return;                                             // wave-uniform
    const vsk::FidPair pr = pairs[VS_IDX((size_t)blockIdx.z, n_pairs, 636)];
    const GPtr<T> ia = (GPtr<T>)pr.a, ib = (GPtr<T>)pr.b;
    const int x0 = (strip * FD_COLS + lane) * 4;                          // the lane's block column
    const int npx = min(max(w - x0, 0), 4);                               // its pixels in a row: 0 past the image
    const bool whole = X4 && npx == 4;
    const bool owns = lane < FD_COLS;                                     // (lane 63's block column is lane 0's of the next strip)
    const bool win_col = owns && x0 + 8 <= w;
    const int br_first = max(br0 - 1, 0), br_end = min(br0 + FD_BAND, (h + 3) >> 2);
    Acc sse[3] = {0, 0, 0};
    uint32_t sse_y = 0, n_win = 0;
    int ssim = 0;
    int prev[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int br = br_first; br < br_end; br++) {
        const bool counts = owns && br >= br0;                            // (the block row above the band: for its windows only)
        uint32_t da[4][ND], db[4][ND];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int y = min(4 * br + r, h - 1);                         // (a row below the image is read as the last one and not used)
            fd_load<T, 630>(ia + VS_IDX((size_t)y * (size_t)a_stride, (long long)(h - 1) * a_stride + 1, 629), x0, npx, w, whole, da[r]);
            fd_load<T, 633>(ib + VS_IDX((size_t)y * (size_t)b_stride, (long long)(h - 1) * b_stride + 1, 632), x0, npx, w, whole, db[r]);
        }
        int blk[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (4 * br + r < h) fd_row<T>(da[r], db[r], npx, maxv, shift, counts, sse, sse_y, blk);       // wave-uniform
        if (br > br_first && 4 * br + 4 <= h) {                           // wave-uniform: block rows br - 1 and br are whole
            int win[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int v = blk[k] + prev[k];
                win[k] = v + __shfl_down(v, 1);
            }
            if (win_col) {
                const int s1 = win[0], s2 = win[1], ss = win[2], s12 = win[3];
                const int vars = 64 * ss - s1 * s1 - s2 * s2, cov = 64 * s12 - s1 * s2;
                const int A = 2 * s1 * s2 + FD_C1, B = 2 * cov + FD_C2, C = s1 * s1 + s2 * s2 + FD_C1, D = vars + FD_C2;
                const double num = (double)((long long)A * (long long)B), den = (double)((long long)C * (long long)D);
                ssim += (int)rint((num / den) * 65536.0);
                n_win++;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) prev[k] = blk[k];
    }
    unsigned long long* const out = stats + (size_t)blockIdx.z * 6;
    const unsigned long long v[6] = {(unsigned long long)sse[0], (unsigned long long)sse[1], (unsigned long long)sse[2], (unsigned long long)sse_y,
                                     (unsigned long long)n_win, (unsigned long long)(long long)ssim};
#pragma unroll
    for (int k = 0; k < 6; k++) {
        unsigned long long sum = v[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0 && sum != 0) atomicAdd(out + VS_IDX(k, 6, 635), sum);
    }
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_fidelity)

namespace vsk {

hipError_t bgr_fidelity(const FidPair* pairs_dev, int w, int h, int a_stride, int b_stride, int bits, int shift_to_8, int max_value, bool on_dwords,
                        unsigned long long* stats, int n_pairs, hipStream_t s) {
    if (!container_ok(bits, max_value) || shift_to_8 < 0 || shift_to_8 > 8 || n_pairs < 1 || w < 1 || h < 1 || w > 32767 || h > 32767 || a_stride < 3 * w ||
        b_stride < 3 * w)
        return hipErrorNotSupported;
    hipError_t e = hipMemsetAsync(stats, 0, (size_t)n_pairs * 6 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const int strips = (((w + 3) & ~3) + FD_STRIP_PX - 1) / FD_STRIP_PX, band_groups = (h + FD_TILE_PX - 1) / FD_TILE_PX;
    for_frame_chunks(n_pairs, [&](int f0, int nf) {                       // gridDim.z limit
        const dim3 grid((unsigned)(strips * band_groups), 1u, (unsigned)nf), block(64 * FD_WAVES);
        const FidPair* pp = pairs_dev + (size_t)f0;
        unsigned long long* sp = stats + (size_t)f0 * 6;
        if (bits == 16 && on_dwords)
            hipLaunchKernelGGL((vs_k_fidelity<uint16_t, true>), grid, block, 0, s, pp, nf, w, h, a_stride, b_stride, shift_to_8, (uint32_t)max_value, sp, strips);
        else if (bits == 16)
            hipLaunchKernelGGL((vs_k_fidelity<uint16_t, false>), grid, block, 0, s, pp, nf, w, h, a_stride, b_stride, shift_to_8, (uint32_t)max_value, sp, strips);
        else if (on_dwords)
            hipLaunchKernelGGL((vs_k_fidelity<uint8_t, true>), grid, block, 0, s, pp, nf, w, h, a_stride, b_stride, shift_to_8, (uint32_t)max_value, sp, strips);
        else
            hipLaunchKernelGGL((vs_k_fidelity<uint8_t, false>), grid, block, 0, s, pp, nf, w, h, a_stride, b_stride, shift_to_8, (uint32_t)max_value, sp, strips);
    });
    return hipGetLastError();
}

}  // namespace vsk
