// vs_inpaint.hip -- what the border fill leaves open, inpainted: a coverage index of the output window and an exact-integer push-pull over it.
// The last-resort spatial pass behind the VS_WARP_BILINEAR_CV warp and its fill (vs_fill.hip); off by default.
//
// THE RULE (also include/vs_amd.h, vs_bgr_fill_coverage_batch / vs_bgr_inpaint_batch; DESIGN.md "Inpaint").  VS_WARP_BILINEAR_CV conventions, 3
// channels, 8- and 16-bit containers, every VS_FMT_BGR*, windows up to 32767 a side.
//   * COVERAGE INDEX.  Output frame o has n_cand (1 .. 16) candidates exactly as in vs_bgr_image_warp_fill_batch: each a forward transform, a
//     negative frame index ends the list, candidate 0 is the frame itself; only the sign of an index is looked at.  For window pixel (x, y),
//     cov = 1 + c, c the first candidate that COVERS the pixel by the fill's int32 rule, unchanged (the positions X, Y from cv_row_origin /
//     cv_delta / cv_pos, saturating cvRound with NaN -> 0, wrapping additions, all four taps inside w x h, full-frame coordinates under the
//     ROI); cov = 0 if no candidate covers it.
//   * INPAINT of one W x H window in place, given a byte mask m0 (non-zero = keep).  Pixel values outside the mask are never read.
//       LEVELS.  W_0 = W, H_0 = H, W_{l+1} = (W_l + 1) >> 1, H_{l+1} = (H_l + 1) >> 1, up to the level L with W_L = H_L = 1.
//       PUSH, l -> l+1, per channel.  The children of (X, Y) are the pixels (2X+i, 2Y+j), i, j in {0, 1}, that exist at level l and have
//         m_l != 0; n their number, s their sum.  n == 0: m_{l+1} = 0, the value is unused.  Otherwise m_{l+1} = 1 and the value is
//         (2 s + n) / (2 n), floor division: the rounded mean; unsigned 32-bit is enough and the result fits the container.
//       If m_L == 0 (no kept pixel in the window) the window is left untouched.
//       PULL, l = L-1 .. 0.  By the time level l is pulled, level l+1 is completely defined.  A pixel (x, y) with m_l == 0 becomes
//         (9 P(px,py) + 3 P(qx,py) + 3 P(px,qy) + P(qx,qy) + 8) >> 4  over level l+1, where px = x >> 1,
//         qx = clamp(px + (x & 1 ? 1 : -1), 0, W_{l+1} - 1), and py, qy the same from y and H_{l+1}.
//     Hence (a) kept pixels come back bit for bit; (b) every inpainted sample lies between the minimum and the maximum of the kept samples of
//     its channel, so max_value never comes into it; (c) kept pixels of one colour give the whole window that colour; (d) an all-kept and an
//     all-open window come back bit for bit; (e) the result does not depend on the prior content of open pixels.
//
// PASSES.  vs_k_fill_coverage is the fill kernel's block / strip walk (vs_cover.hpp: one copy of cv_covers_rect): a 256 x 256 block or a 64 x 16
// strip that candidate 0 covers is stored as 1s, with dword stores where the rows of the index start on dwords; elsewhere a lane walks the
// candidates in a wave-uniform loop -- candidates outside, the strip's rows inside: an entry is read once per strip -- and stores its byte.
// Every wave sums its lanes' open pixels and adds them to the frame's count: one vector atomic per wave.  Level 0 of the pyramid is the
// window itself with its byte mask; the levels above are texels of four container-sized elements B, G, R, m (4 or 8 bytes, aligned loads
// and stores) in a scratch of about 4/3 of a texel per four pixels.  One
// push launch and one pull launch per full-size level over all frames of the group; from the first level of at most kTailTexels texels on,
// one "tail" workgroup per frame takes that level into LDS, goes the rest of the way down and back up there and hands the level back,
// completely defined.  (A level below a 1 x N level has N / 2 texels, not N / 4: the levels from the tail level down hold at most 2 * 4096 of
// them, 64 KB of 16-bit texels; the launcher starts the tail one level later where a shape would ask for more.)  Every kernel leaves at once
// for a frame whose open count is 0 or the window size: such a window comes back untouched.  A lane owns adjacent texels: neighbouring lanes
// read neighbouring 6- or 12-byte pixel pairs of level 0, and neighbouring aligned texels above.
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cover.hpp"
#include "vs_launch.hpp"

using namespace vsd;

namespace {

constexpr int IP_THREADS = 256;                            // push / pull / count: one thread per texel of the level written
constexpr int kTailTexels = 4096;                          // the tail starts at the first level with at most this many texels ...
constexpr int kTailLds = 2 * kTailTexels;                  // ... and holds that level and every level below it in LDS
constexpr int TAIL_THREADS = 512;

template <typename T> struct alignas(4 * sizeof(T)) Tex { T b, g, r, m; };

// nx x ny bytes of 1 at (x0, y0) of the index, by `nt` threads of which this is `tid`.  wide: the index's rows start on dwords and x0 is a
// multiple of 4, so whole groups of four go out as one dword.  Sites 561 / 562: the last byte of a store lies inside the index.
__device__ __forceinline__ void store_ones(uint8_t* __restrict__ cov, int cov_stride, long long extent, int x0, int y0, int nx, int ny, int tid, int nt, bool wide) {
    (void)extent;
    const int per_row = (nx + 3) >> 2, total = per_row * ny;
    for (int i = tid; i < total; i += nt) {
        const int r = i / per_row, d = i - r * per_row;
        const long long at = (long long)(y0 + r) * cov_stride + x0 + 4 * d;
        if (wide && 4 * d + 4 <= nx) {
            *(uint32_t*)(cov + VS_IDX(at, extent - 3, 561)) = 0x01010101u;
        } else {
            for (int k = 0; k < 4 && 4 * d + k < nx; k++) cov[VS_IDX(at + k, extent, 562)] = 1;
        }
    }
}

// cands: n_cand entries per output frame (gridDim.y frames) as the fill kernel takes them: entry 0's matrix is the frame's own, a null frame
// ends the list (the frames are not read: only whether an entry has one).  open_count (may be null): += the frame's pixels without a candidate.
__global__ __launch_bounds__(64 * FL_WAVES) void vs_k_fill_coverage(const vsk::FillCand* __restrict__ cands, int n_cand, int w, int h, uint8_t* __restrict__ cov,
                                                                  int cov_stride, size_t cov_fs, vsk::Roi roi, int blocks_x, int wide,
                                                                  unsigned int* __restrict__ open_count) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int byi = (int)blockIdx.x / blocks_x, bxi = (int)blockIdx.x - byi * blocks_x;
    const int bx0 = bxi * FL_BLOCK, by0 = byi * FL_BLOCK;                  // this workgroup's block in the output window
    cands += (size_t)blockIdx.y * (size_t)n_cand;
    cov += (size_t)blockIdx.y * cov_fs;
    const long long extent = (long long)(roi.h - 1) * cov_stride + roi.w;  // bytes of a frame's index
    double M[6];
#pragma unroll
    for (int k = 0; k < 6; k++) M[k] = cands[0].m[k];
    const int bnx = min(FL_BLOCK, roi.w - bx0), bny = min(FL_BLOCK, roi.h - by0);
    if (cv_covers_rect(M, roi, bx0, by0, bnx, bny, w, h)) {                // uniform
        store_ones(cov, cov_stride, extent, bx0, by0, bnx, bny, (int)threadIdx.x, 64 * FL_WAVES, wide != 0);
        return;
    }
    unsigned int n_open = 0;                                               // this lane's open pixels
#pragma unroll 1
    for (int t = 0; t < (FL_BLOCK / FL_W) * (FL_BLOCK / (FL_ROWS * FL_WAVES)); t++) {
        const int x0 = bx0 + (t % (FL_BLOCK / FL_W)) * FL_W, y0 = by0 + ((t / (FL_BLOCK / FL_W)) * FL_WAVES + wv) * FL_ROWS;     // this wave's strip
        if (x0 >= roi.w || y0 >= roi.h) continue;                          // wave-uniform
        const int nx = min(FL_W, roi.w - x0), ny = min(FL_ROWS, roi.h - y0);  // live columns / rows (>= 1)
        if (cv_covers_rect(M, roi, x0, y0, nx, ny, w, h)) {                // wave-uniform
            store_ones(cov, cov_stride, extent, x0, y0, nx, ny, lane, 64, wide != 0);
            continue;
        }
        const int x = x0 + lane;
        const bool lane_in = lane < nx;
        const int fx = min(x, roi.w - 1) + roi.x;
        // A lane owns its column of the strip: candidate 0 first, row by row (1 or 0 stored, the open rows kept as bits); then the candidates
        // in order, each entry read once per strip (scalar loads) and asked about the rows that are still open -- the first that covers a pixel
        // overwrites its 0.  (The fill walks rows outside and candidates inside; here nothing is sampled, so the entry's loads and the
        // candidate's two column terms leave the row loop.)  Site 563: the pixel's byte lies inside the index.
        unsigned int open_rows = 0;
        {
            const int ad0 = cv_delta(M[0], fx), bd0 = cv_delta(M[3], fx);
            for (int r = 0; r < ny; r++) {
                const int y = y0 + r, fy = y + roi.y;
                const bool c0 = cv_covers(cv_pos(cv_row_origin(M[1], M[2], fy), cv_row_origin(M[4], M[5], fy), ad0, bd0), w, h);
                if (lane_in) {
                    cov[VS_IDX((long long)y * cov_stride + x, extent, 563)] = c0 ? 1 : 0;
                    if (!c0) open_rows |= 1u << r;
                }
            }
        }
#pragma unroll 1
        for (int c = 1; c < n_cand; c++) {                   // wave-uniform
            if (__builtin_amdgcn_ballot_w64(open_rows != 0u) == 0) break;
            if (!cands[c].src) break;
            double C[6];
#pragma unroll
            for (int k = 0; k < 6; k++) C[k] = cands[c].m[k];
            const int adc = cv_delta(C[0], fx), bdc = cv_delta(C[3], fx);
            for (int r = 0; r < ny; r++) {
                const bool open = ((open_rows >> r) & 1u) != 0u;
                if (__builtin_amdgcn_ballot_w64(open) == 0) continue;      // wave-uniform
                const int y = y0 + r, fy = y + roi.y;
                if (open && cv_covers(cv_pos(cv_row_origin(C[1], C[2], fy), cv_row_origin(C[4], C[5], fy), adc, bdc), w, h)) {
                    cov[VS_IDX((long long)y * cov_stride + x, extent, 563)] = (uint8_t)(1 + c);
                    open_rows &= ~(1u << r);
                }
            }
        }
        n_open += (unsigned int)__popc(open_rows);
    }
    if (open_count) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) n_open += __shfl_xor(n_open, off);
        if (lane == 0 && n_open != 0) atomicAdd(open_count + blockIdx.y, n_open);
    }
}

// counts[frame] (zeroed by the launcher on the same stream) += the zero bytes of the frame's mask; a workgroup owns 16 rows
__global__ __launch_bounds__(IP_THREADS) void vs_k_mask_open_count(const uint8_t* __restrict__ mask, int w, int h, int mask_stride, size_t mask_fs,
                                                                   unsigned int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    mask += (size_t)blockIdx.y * mask_fs;
    const long long extent = (long long)(h - 1) * mask_stride + w;
    (void)extent;
    const int y0 = (int)blockIdx.x * 16, y1 = min(y0 + 16, h);
    unsigned int n_open = 0;                                               // wave-uniform
    for (int y = y0; y < y1; y++)
        for (int xb = 0; xb < w; xb += IP_THREADS) {
            const int x = xb + (int)threadIdx.x;
            const bool open = x < w && mask[VS_IDX((long long)y * mask_stride + min(x, w - 1), extent, 564)] == 0;
            n_open += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(open));
        }
    if (lane == 0 && n_open != 0) atomicAdd(counts + blockIdx.y, n_open);
}

// ---- the rule's two sentences, on whatever holds a level --------------------------------------------------------------------
struct Acc { uint32_t n, b, g, r; };
template <typename T> __device__ __forceinline__ void acc_add(Acc& a, Tex<T> t) {
    if (t.m != 0) { a.n++; a.b += t.b; a.g += t.g; a.r += t.r; }
}
template <typename T> __device__ __forceinline__ Tex<T> push_value(const Acc& a) {
    if (a.n == 0) return Tex<T>{0, 0, 0, 0};
    const uint32_t d = 2u * a.n;
    return Tex<T>{(T)((2u * a.b + a.n) / d), (T)((2u * a.g + a.n) / d), (T)((2u * a.r + a.n) / d), (T)1};
}
// where pixel (x, y) of level l looks in level l+1 (W1 x H1): the near texel and its neighbour towards the pixel's side, clamped
struct Taps { int px, qx, py, qy; };
__device__ __forceinline__ Taps pull_taps(int x, int y, int W1, int H1) {
    const int px = x >> 1, py = y >> 1;
    return Taps{px, clampi(px + ((x & 1) ? 1 : -1), 0, W1 - 1), py, clampi(py + ((y & 1) ? 1 : -1), 0, H1 - 1)};
}
template <typename T> __device__ __forceinline__ Tex<T> pull_value(Tex<T> pp, Tex<T> qp, Tex<T> pq, Tex<T> qq) {
    return Tex<T>{(T)((9u * pp.b + 3u * qp.b + 3u * pq.b + qq.b + 8u) >> 4), (T)((9u * pp.g + 3u * qp.g + 3u * pq.g + qq.g + 8u) >> 4),
                  (T)((9u * pp.r + 3u * qp.r + 3u * pq.r + qq.r + 8u) >> 4), (T)1};
}

// a frame that has nothing to do: no open pixel, or no kept one
__device__ __forceinline__ bool frame_idle(const unsigned int* __restrict__ counts, unsigned int total) {
    const unsigned int c = counts[blockIdx.y];
    return c == 0u || c >= total;
}

// level 0 as texels: pixel (x, y) of the window with its mask byte; the samples of an open pixel are not read.  Sites 565 / 566: the mask byte and
// the pixel's last sample lie inside the mask / the window
template <typename T>
__device__ __forceinline__ Tex<T> window_texel(const T* __restrict__ img, int stride, const uint8_t* __restrict__ mask, int mask_stride, int x, int y, int W, int H) {
    (void)W; (void)H;
    if (mask[VS_IDX((long long)y * mask_stride + x, (long long)(H - 1) * mask_stride + W, 565)] == 0) return Tex<T>{0, 0, 0, 0};
    const T* const px = img + VS_IDX((long long)y * stride + 3LL * x, (long long)(H - 1) * stride + 3LL * W - 2, 566);
    return Tex<T>{px[0], px[1], px[2], (T)1};
}

// PUSH l -> l+1 in global memory: one thread per texel of level l+1 (W1 x H1), gridDim.y frames.  L0: level l is the window and its mask;
// else Wl x Hl texels at `src`.  Every texel of level l+1 is written.  Sites 567 / 568: pyramid reads and writes.
template <typename T, bool L0>
__global__ __launch_bounds__(IP_THREADS) void vs_k_inpaint_push(const T* __restrict__ img, int stride, size_t img_fs, const uint8_t* __restrict__ mask, int mask_stride,
                                                                size_t mask_fs, const Tex<T>* __restrict__ src, Tex<T>* __restrict__ dst, size_t pyr_fs, int Wl, int Hl,
                                                                const unsigned int* __restrict__ counts, unsigned int total) {
    if (frame_idle(counts, total)) return;
    const int W1 = (Wl + 1) >> 1, H1 = (Hl + 1) >> 1;
    const long long i = (long long)blockIdx.x * IP_THREADS + threadIdx.x;
    if (i >= (long long)W1 * H1) return;
    const int Y = (int)(i / W1), X = (int)(i - (long long)Y * W1);
    if (L0) { img += (size_t)blockIdx.y * img_fs; mask += (size_t)blockIdx.y * mask_fs; }
    else src += (size_t)blockIdx.y * pyr_fs;
    dst += (size_t)blockIdx.y * pyr_fs;
    Acc a{0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int cx = 2 * X + k, cy = 2 * Y + j;
            if (cx < Wl && cy < Hl) acc_add(a, L0 ? window_texel(img, stride, mask, mask_stride, cx, cy, Wl, Hl) : src[VS_IDX((long long)cy * Wl + cx, (long long)Wl * Hl, 567)]);
        }
    dst[VS_IDX(i, (long long)W1 * H1, 568)] = push_value<T>(a);
}

// PULL of level l (Wl x Hl) from level l+1 at `up`, completely defined: one thread per texel of level l.  L0: level l is the window, whose open
// pixels are stored (site 571: the store's last sample lies inside the window); else the texels at `lvl`, whose undefined ones become defined.
// Sites 569 / 570: pyramid reads and writes.
template <typename T, bool L0>
__global__ __launch_bounds__(IP_THREADS) void vs_k_inpaint_pull(T* __restrict__ img, int stride, size_t img_fs, const uint8_t* __restrict__ mask, int mask_stride,
                                                                size_t mask_fs, Tex<T>* __restrict__ lvl, const Tex<T>* __restrict__ up, size_t pyr_fs, int Wl, int Hl,
                                                                const unsigned int* __restrict__ counts, unsigned int total) {
    if (frame_idle(counts, total)) return;
    const int W1 = (Wl + 1) >> 1, H1 = (Hl + 1) >> 1;
    const long long i = (long long)blockIdx.x * IP_THREADS + threadIdx.x;
    if (i >= (long long)Wl * Hl) return;
    const int y = (int)(i / Wl), x = (int)(i - (long long)y * Wl);
    up += (size_t)blockIdx.y * pyr_fs;
    if (L0) {
        mask += (size_t)blockIdx.y * mask_fs;
        if (mask[VS_IDX((long long)y * mask_stride + x, (long long)(Hl - 1) * mask_stride + Wl, 565)] != 0) return;
    } else {
        lvl += (size_t)blockIdx.y * pyr_fs;
        if (lvl[VS_IDX(i, (long long)Wl * Hl, 569)].m != 0) return;
    }
    const Taps t = pull_taps(x, y, W1, H1);
    const long long n1 = (long long)W1 * H1;
    (void)n1;
    const Tex<T> v = pull_value(up[VS_IDX((long long)t.py * W1 + t.px, n1, 569)], up[VS_IDX((long long)t.py * W1 + t.qx, n1, 569)],
                                up[VS_IDX((long long)t.qy * W1 + t.px, n1, 569)], up[VS_IDX((long long)t.qy * W1 + t.qx, n1, 569)]);
    if (L0) {
        T* const px = img + (size_t)blockIdx.y * img_fs + VS_IDX((long long)y * stride + 3LL * x, (long long)(Hl - 1) * stride + 3LL * Wl - 2, 571);
        px[0] = v.b; px[1] = v.g; px[2] = v.r;
    } else {
        lvl[VS_IDX(i, (long long)Wl * Hl, 570)] = v;
    }
}

// level k below the tail level (Wt x Ht): its size and where it starts in the tail's LDS
__device__ __forceinline__ void tail_level(int Wt, int Ht, int k, int* W, int* H, int* off) {
    int w = Wt, h = Ht, o = 0;
    for (int q = 0; q < k; q++) { o += w * h; w = (w + 1) >> 1; h = (h + 1) >> 1; }
    *W = w; *H = h; *off = o;
}

// THE TAIL: one workgroup per frame.  The tail level (Wt x Ht <= kTailTexels texels; from_image: the window and its mask, else the texels at
// `lvl`) goes into LDS, the levels below it are pushed there down to 1 x 1 and pulled back up, and the tail level leaves completely defined
// (from_image: the window's open pixels are stored).  Every LDS index through VS_IDX against kTailLds (sites 572 - 575).
template <typename T>
__global__ __launch_bounds__(TAIL_THREADS) void vs_k_inpaint_tail(T* __restrict__ img, int stride, size_t img_fs, const uint8_t* __restrict__ mask, int mask_stride,
                                                                  size_t mask_fs, Tex<T>* __restrict__ lvl, size_t pyr_fs, int Wt, int Ht, int from_image,
                                                                  const unsigned int* __restrict__ counts, unsigned int total) {
    __shared__ Tex<T> lds[kTailLds];
    if (frame_idle(counts, total)) return;                                 // uniform
    const int tid = (int)threadIdx.x, nt = Wt * Ht;
    if (from_image) { img += (size_t)blockIdx.y * img_fs; mask += (size_t)blockIdx.y * mask_fs; }
    else lvl += (size_t)blockIdx.y * pyr_fs;
    for (int i = tid; i < nt; i += TAIL_THREADS) {
        Tex<T> t;
        if (from_image) { const int y = i / Wt; t = window_texel(img, stride, mask, mask_stride, i - y * Wt, y, Wt, Ht); }
        else t = lvl[VS_IDX(i, nt, 567)];
        lds[VS_IDX(i, kTailLds, 572)] = t;
    }
    __syncthreads();
    int levels = 0;                                                        // levels below the tail level
    for (int W = Wt, H = Ht, off = 0; W > 1 || H > 1; levels++) {
        const int W1 = (W + 1) >> 1, H1 = (H + 1) >> 1, off1 = off + W * H;
        for (int i = tid; i < W1 * H1; i += TAIL_THREADS) {
            const int Y = i / W1, X = i - Y * W1;
            Acc a{0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int cx = 2 * X + k, cy = 2 * Y + j;
                    if (cx < W && cy < H) acc_add(a, lds[VS_IDX(off + cy * W + cx, kTailLds, 573)]);
                }
            lds[VS_IDX(off1 + i, kTailLds, 574)] = push_value<T>(a);
        }
        __syncthreads();
        W = W1; H = H1; off = off1;
    }
    // (the 1 x 1 level is defined: the frame has a kept pixel, or it would have been idle)
    for (int k = levels - 1; k >= 0; k--) {
        int W, H, off;
        tail_level(Wt, Ht, k, &W, &H, &off);
        const int W1 = (W + 1) >> 1, H1 = (H + 1) >> 1, off1 = off + W * H;
        for (int i = tid; i < W * H; i += TAIL_THREADS) {
            if (lds[VS_IDX(off + i, kTailLds, 575)].m != 0) continue;
            const int y = i / W;
            const Taps t = pull_taps(i - y * W, y, W1, H1);
            lds[VS_IDX(off + i, kTailLds, 575)] = pull_value(lds[VS_IDX(off1 + t.py * W1 + t.px, kTailLds, 575)], lds[VS_IDX(off1 + t.py * W1 + t.qx, kTailLds, 575)],
                                                             lds[VS_IDX(off1 + t.qy * W1 + t.px, kTailLds, 575)], lds[VS_IDX(off1 + t.qy * W1 + t.qx, kTailLds, 575)]);
        }
        __syncthreads();
    }
    for (int i = tid; i < nt; i += TAIL_THREADS) {
        const Tex<T> t = lds[VS_IDX(i, kTailLds, 572)];
        if (from_image) {
            const int y = i / Wt, x = i - y * Wt;
            if (mask[VS_IDX((long long)y * mask_stride + x, (long long)(Ht - 1) * mask_stride + Wt, 565)] != 0) continue;
            T* const px = img + VS_IDX((long long)y * stride + 3LL * x, (long long)(Ht - 1) * stride + 3LL * Wt - 2, 571);
            px[0] = t.b; px[1] = t.g; px[2] = t.r;
        } else {
            lvl[VS_IDX(i, nt, 568)] = t;
        }
    }
}

// the levels of a W x H window: sizes, the level the tail starts at, where the levels 1 .. tail lie in a frame's pyramid (texels)
struct Plan { int n_levels, tail; int W[17], H[17]; size_t off[17], texels; };
Plan make_plan(int w, int h) {
    Plan p{};
    p.W[0] = w; p.H[0] = h; p.n_levels = 1;
    while (p.W[p.n_levels - 1] > 1 || p.H[p.n_levels - 1] > 1) {
        p.W[p.n_levels] = (p.W[p.n_levels - 1] + 1) >> 1; p.H[p.n_levels] = (p.H[p.n_levels - 1] + 1) >> 1; p.n_levels++;
    }
    auto below = [&](int l) { size_t t = 0; for (int k = l; k < p.n_levels; k++) t += (size_t)p.W[k] * p.H[k]; return t; };
    p.tail = 0;
    while ((size_t)p.W[p.tail] * p.H[p.tail] > (size_t)kTailTexels || below(p.tail) > (size_t)kTailLds) p.tail++;     // (the 1 x 1 level satisfies both)
    for (int l = 1; l <= p.tail; l++) { p.off[l] = p.texels; p.texels += (size_t)p.W[l] * p.H[l]; }
    return p;
}

template <typename T>
hipError_t inpaint_launch(T* img, size_t img_fs, int n, int w, int h, int stride, const uint8_t* mask, size_t mask_fs, int mask_stride, const unsigned int* counts,
                          Tex<T>* pyr, hipStream_t s) {
    const Plan p = make_plan(w, h);
    const unsigned int total = (unsigned int)((size_t)w * h);
    auto blocks = [](int W, int H) { return (unsigned)(((size_t)W * H + IP_THREADS - 1) / IP_THREADS); };
    vsk::for_frame_chunks(n, [&](int f0, int count) {
        const unsigned nf = (unsigned)count;
        T* const ip = img + (size_t)f0 * img_fs;
        const uint8_t* const mp = mask + (size_t)f0 * mask_fs;
        Tex<T>* const pp = pyr + (size_t)f0 * p.texels;
        const unsigned int* const cp = counts + f0;
        for (int l = 0; l < p.tail; l++) {
            const dim3 grid(blocks(p.W[l + 1], p.H[l + 1]), nf);
            if (l == 0)
                hipLaunchKernelGGL((vs_k_inpaint_push<T, true>), grid, dim3(IP_THREADS), 0, s, ip, stride, img_fs, mp, mask_stride, mask_fs, (const Tex<T>*)nullptr, pp + p.off[1],
                                   p.texels, p.W[0], p.H[0], cp, total);
            else
                hipLaunchKernelGGL((vs_k_inpaint_push<T, false>), grid, dim3(IP_THREADS), 0, s, (const T*)nullptr, 0, (size_t)0, (const uint8_t*)nullptr, 0, (size_t)0,
                                   (const Tex<T>*)(pp + p.off[l]), pp + p.off[l + 1], p.texels, p.W[l], p.H[l], cp, total);
        }
        hipLaunchKernelGGL(vs_k_inpaint_tail<T>, dim3(1, nf), dim3(TAIL_THREADS), 0, s, ip, stride, img_fs, mp, mask_stride, mask_fs, p.tail ? pp + p.off[p.tail] : (Tex<T>*)nullptr,
                           p.texels, p.W[p.tail], p.H[p.tail], p.tail == 0 ? 1 : 0, cp, total);
        for (int l = p.tail - 1; l >= 0; l--) {
            const dim3 grid(blocks(p.W[l], p.H[l]), nf);
            if (l == 0)
                hipLaunchKernelGGL((vs_k_inpaint_pull<T, true>), grid, dim3(IP_THREADS), 0, s, ip, stride, img_fs, mp, mask_stride, mask_fs, (Tex<T>*)nullptr,
                                   (const Tex<T>*)(pp + p.off[1]), p.texels, p.W[0], p.H[0], cp, total);
            else
                hipLaunchKernelGGL((vs_k_inpaint_pull<T, false>), grid, dim3(IP_THREADS), 0, s, (T*)nullptr, 0, (size_t)0, (const uint8_t*)nullptr, 0, (size_t)0, pp + p.off[l],
                                   (const Tex<T>*)(pp + p.off[l + 1]), p.texels, p.W[l], p.H[l], cp, total);
        }
    });
    return hipGetLastError();
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_inpaint)

namespace vsk {

hipError_t fill_coverage(const FillCand* cands_dev, int n_cand, int w, int h, uint8_t* cov, int cov_stride, int n_frames, size_t cov_fs, Roi roi,
                         unsigned int* open_count, hipStream_t s) {
    if (w > 32767 || h > 32767 || n_cand < 1 || roi.w < 1 || roi.h < 1) return hipErrorNotSupported;
    const int blocks_x = (roi.w + FL_BLOCK - 1) / FL_BLOCK, blocks_y = (roi.h + FL_BLOCK - 1) / FL_BLOCK;
    // dword stores where every row of every frame's index starts on a dword
    const int wide = rows_on_dwords(cov, cov_stride, cov_fs, n_frames, 1);
    if (open_count) {
        const hipError_t e = hipMemsetAsync(open_count, 0, (size_t)n_frames * sizeof(unsigned int), s);
        if (e != hipSuccess) return e;
    }
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        hipLaunchKernelGGL(vs_k_fill_coverage, dim3((unsigned)(blocks_x * blocks_y), (unsigned)nf), dim3(64 * FL_WAVES), 0, s, cands_dev + (size_t)f0 * (size_t)n_cand, n_cand,
                           w, h, cov + (size_t)f0 * cov_fs, cov_stride, cov_fs, roi, blocks_x, wide, open_count ? open_count + f0 : nullptr);
    });
    return hipGetLastError();
}

size_t inpaint_pyramid_bytes(int w, int h, int bits) {
    return make_plan(w, h).texels * 4 * (size_t)(bits / 8);
}

hipError_t mask_open_count(const uint8_t* mask, int w, int h, int mask_stride, size_t mask_fs, int n_frames, unsigned int* counts, hipStream_t s) {
    if (w < 1 || h < 1 || n_frames < 1) return hipErrorNotSupported;
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_frames * sizeof(unsigned int), s);
    if (e != hipSuccess) return e;
    for_frame_chunks(n_frames, [&](int f0, int nf) {
        hipLaunchKernelGGL(vs_k_mask_open_count, dim3((unsigned)((h + 15) / 16), (unsigned)nf), dim3(IP_THREADS), 0, s, mask + (size_t)f0 * mask_fs, w, h, mask_stride, mask_fs,
                           counts + f0);
    });
    return hipGetLastError();
}

hipError_t bgr_inpaint(void* img, size_t img_fs, int n_frames, int w, int h, int stride, int bits, const uint8_t* mask, size_t mask_fs, int mask_stride,
                       const unsigned int* counts, void* pyramid, hipStream_t s) {
    if ((bits != 8 && bits != 16) || w < 1 || h < 1 || w > 32767 || h > 32767 || n_frames < 1) return hipErrorNotSupported;
    if (bits == 16) return inpaint_launch<uint16_t>((uint16_t*)img, img_fs, n_frames, w, h, stride, mask, mask_fs, mask_stride, counts, (Tex<uint16_t>*)pyramid, s);
    return inpaint_launch<uint8_t>((uint8_t*)img, img_fs, n_frames, w, h, stride, mask, mask_fs, mask_stride, counts, (Tex<uint8_t>*)pyramid, s);
}

}  // namespace vsk
