// vs_flow.hip -- dense optical flow on gfx950 and the flow-based jitter score (eval_jitter.cpp:43-70,
// grid_search_align.cpp:27-60: cv::calcOpticalFlowFarneback(prev, next, flow, 0.5, 3, 15, 3, 5, 1.2, 0), element n/2 of the
// per-pixel magnitudes per frame pair, the median over pairs).
//
// OpenCV is not part of this build and its exact arithmetic is not pinned here, so the algorithm -- two-frame polynomial
// expansion flow (Farneback 2003) with OpenCV's parameter meanings -- is specified by this build.  tests/_flow_ref.py restates
// the specification in numpy float32 in the kernels' operation order; the kernels equal it bit for bit.  Choices of this build:
//
//   Layers      levels + 1 layers, k = 0..levels (levels = 0: the frame alone).  scale_k = pyr_scale multiplied k times (double);
//               w_k = max(1, floor(w * scale_k + 0.5)), h_k likewise.  Every layer is used, down to 1 x 1.
//   Pyramid     layer 0 = the u8 frame as float.  Layer k > 0: level 0 blurred by a normalised Gaussian of sigma = (1/scale_k - 1)/2
//               over offsets -r..r, r = max(1, ceil(3 sigma)) (at most kMaxPyrR), vertically then horizontally, then sampled
//               bilinearly at ((x + 0.5) * w/w_k - 0.5, ...), the coordinate clamped to [0, w-1] (the ratio rounded to float once).
//   Expansion   separable over offsets -poly_n..poly_n with a normalised Gaussian of sigma = poly_sigma: vertical sums of g, g*t,
//               g*t^2, then horizontal sums to the six moments; the weighted least-squares fit of {1, x, y, x^2, y^2, xy} reduces
//               to five constants of the inverse Gram matrix (ig11, ig03, ig33, ig34, ig55) computed on the host in double.
//               Output per pixel: b1, b2, a11, a22, a12 (the quadratic form's off-diagonal, i.e. half the xy coefficient).
//   Borders     every neighbourhood read (pyramid blur, expansion, box window, bilinear samples) clamps the coordinate to the
//               layer (replicated border).  No border weighting of the matrices.
//   Update      A = (A_prev(x) + A_next(x + d)) / 2, db = (b_prev(x) - b_next(x + d)) / 2 + A d, the next frame's coefficients
//               sampled bilinearly at x + d clamped to [0, w_k - 1]; entries A^T A (3) and A^T db (2).  The first update of a
//               layer uses the coarser layer's flow resampled like the pyramid and multiplied by 1/pyr_scale (zero on the top layer).
//   Solve       winsize x winsize box SUM (vertical, then horizontal; offsets -(winsize/2) .. winsize-1-winsize/2) of the five
//               planes, then d = adj(G) h / (max(det G, 0) + 1e-3).  `iterations` solves per layer; every solve but the last is
//               followed by the next update in the same kernel.
//   Statistic   per pair, element n/2 (n = w*h) of dx*dx + dy*dy selected exactly on the device (radix select on the float bits,
//               11 + 11 + 10 bits), then one correctly rounded sqrtf on the host; the clip score is the median over pairs
//               (the mean of the two middle values for an even count), in double.
// Numerics: every product and sum one fp32 rounding (-ffp-contract=off, no fma anywhere), sums over taps in ascending order
// from 0.0f, correctly rounded division; Gaussian weights and inverse-G constants are made on the host (no device expf).
//
// Shape of the work: every stage is one launch over all frames (grid z = frame) or all pairs (grid z = pair) of a chunk, and a
// frame's expansion is made once per layer and read by both of its pairs.  Clips run in chunks of frames whose scratch fits
// kMemCap, consecutive chunks sharing one frame.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "vs_device.hpp"
#include "vs_internal.hpp"
#include "vs_kernels.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 16;                 // output tile of the LDS kernels: 64 x 16 pixels, 4 per thread
constexpr int kMaxPyrR = 128;                     // longest pyramid blur half-width
constexpr int kMaxPolyN = 7;
constexpr int kMaxWin = 31;
constexpr int kHistBins = 2048;
constexpr size_t kMemCap = (size_t)2 << 30;       // scratch of one chunk (soft: a chunk always holds one pair)

struct PyrTaps { float v[2 * kMaxPyrR + 1]; };
struct PolyConsts { float g[2 * kMaxPolyN + 1], gt[2 * kMaxPolyN + 1], gtt[2 * kMaxPolyN + 1]; float ig11, ig03, ig33, ig34, ig55; };
struct SelState { uint32_t prefix, k; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// centre-aligned source coordinate of output sample i, clamped to [0, n_in - 1]: i0, i1, t
__device__ __forceinline__ void src_coord(int i, float ratio, int n_in, int& i0, int& i1, float& t) {
    float s = ((float)i + 0.5f) * ratio - 0.5f;
    s = fminf(fmaxf(s, 0.0f), (float)(n_in - 1));
    i0 = (int)s;
    i1 = min(i0 + 1, n_in - 1);
    t = s - (float)i0;
}

__device__ __forceinline__ float bilerp(float p00, float p10, float p01, float p11, float tx, float ty) {
    const float u = 1.0f - tx, v = 1.0f - ty;
    const float top = p00 * u + p10 * tx;
    const float bot = p01 * u + p11 * tx;
    return top * v + bot * ty;
}

// ---- pyramid ------------------------------------------------------------------------------------------------------------
// vertical Gaussian of level 0 (u8, any stride) -> f32 w x h, frame = blockIdx.z
__global__ __launch_bounds__(kThreads) void vs_k_flow_vblur(const uint8_t* __restrict__ src, size_t src_fs, int stride, int w, int h,
                                                            PyrTaps taps, int r, float* __restrict__ dst, size_t dst_fs) {
    const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    src += blockIdx.z * src_fs;
    float acc = 0.0f;
    for (int i = 0; i <= 2 * r; i++) acc = acc + taps.v[i] * (float)src[(size_t)clampi(y - r + i, 0, h - 1) * stride + x];
    dst[blockIdx.z * dst_fs + (size_t)y * w + x] = acc;
}

// horizontal Gaussian of the vertical pass at the four bilinear taps of each layer pixel -> layer k (dense w_k x h_k)
__device__ __forceinline__ float hblur_at(const float* __restrict__ row, int x, int w, const PyrTaps& taps, int r) {
    float acc = 0.0f;
    for (int i = 0; i <= 2 * r; i++) acc = acc + taps.v[i] * row[clampi(x - r + i, 0, w - 1)];
    return acc;
}
__global__ __launch_bounds__(kThreads) void vs_k_flow_hblur_resize(const float* __restrict__ V, size_t v_fs, int w, int h, PyrTaps taps, int r,
                                                                   float rx, float ry, float* __restrict__ L, size_t l_fs, int wk, int hk) {
    const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
    if (x >= wk) return;
    V += blockIdx.z * v_fs;
    int x0, x1, y0, y1;
    float tx, ty;
    src_coord(x, rx, w, x0, x1, tx);
    src_coord(y, ry, h, y0, y1, ty);
    const float* r0 = V + (size_t)y0 * w;
    const float* r1 = V + (size_t)y1 * w;
    const float p00 = hblur_at(r0, x0, w, taps, r), p10 = hblur_at(r0, x1, w, taps, r);
    const float p01 = hblur_at(r1, x0, w, taps, r), p11 = hblur_at(r1, x1, w, taps, r);
    L[blockIdx.z * l_fs + (size_t)y * wk + x] = bilerp(p00, p10, p01, p11, tx, ty);
}

// ---- polynomial expansion -----------------------------------------------------------------------------------------------
// One 64 x 16 output tile per workgroup: the tile + halo of the layer in LDS, the three vertical moments of every halo column,
// then the six horizontal moments per pixel.  coef: 5 planes (b1, b2, a11, a22, a12) of w x h per frame.
constexpr int kPolyPitch = kTW + 2 * kMaxPolyN;                 // 78 floats: rows of the staged tile
constexpr int kPolyTile = (kTH + 2 * kMaxPolyN) * kPolyPitch, kPolyVm = kTH * kPolyPitch;
template <typename T>
__global__ __launch_bounds__(kThreads) void vs_k_flow_polyexp(const T* __restrict__ src, size_t src_fs, int stride, int w, int h, int n,
                                                              PolyConsts pc, float* __restrict__ coef, size_t coef_fs) {
    __shared__ float tile[kPolyTile];
    __shared__ float vm[3][kPolyVm];
    src += blockIdx.z * src_fs;
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, tid = threadIdx.x;
    const int cols = kTW + 2 * n, rows = kTH + 2 * n;
    for (int i = tid; i < rows * cols; i += kThreads) {
        const int r = i / cols, c = i - r * cols;
        const int gy = clampi(y0 - n + r, 0, h - 1), gx = clampi(x0 - n + c, 0, w - 1);
        tile[VS_IDX(r * kPolyPitch + c, kPolyTile, 401)] = (float)src[(size_t)gy * stride + gx];
    }
    __syncthreads();
    for (int i = tid; i < kTH * cols; i += kThreads) {
        const int r = i / cols, c = i - r * cols;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
        for (int t = 0; t <= 2 * n; t++) {
            const float v = tile[VS_IDX((r + t) * kPolyPitch + c, kPolyTile, 402)];
            s0 = s0 + pc.g[t] * v;
            s1 = s1 + pc.gt[t] * v;
            s2 = s2 + pc.gtt[t] * v;
        }
        vm[0][VS_IDX(r * kPolyPitch + c, kPolyVm, 403)] = s0;
        vm[1][VS_IDX(r * kPolyPitch + c, kPolyVm, 403)] = s1;
        vm[2][VS_IDX(r * kPolyPitch + c, kPolyVm, 403)] = s2;
    }
    __syncthreads();
    const int c = tid % kTW, x = x0 + c;
    const size_t plane = (size_t)w * h;
    float* out = coef + blockIdx.z * coef_fs;
    for (int j = 0; j < kTH / (kThreads / kTW); j++) {
        const int r = tid / kTW + j * (kThreads / kTW), y = y0 + r;
        float h0 = 0.0f, hx = 0.0f, hxx = 0.0f, hy = 0.0f, hyy = 0.0f, hxy = 0.0f;
        for (int s = 0; s <= 2 * n; s++) {
            const int vi = VS_IDX(r * kPolyPitch + c + s, kPolyVm, 404);
            const float v0 = vm[0][vi], v1 = vm[1][vi], v2 = vm[2][vi];
            h0 = h0 + pc.g[s] * v0;
            hx = hx + pc.gt[s] * v0;
            hxx = hxx + pc.gtt[s] * v0;
            hy = hy + pc.g[s] * v1;
            hyy = hyy + pc.g[s] * v2;
            hxy = hxy + pc.gt[s] * v1;
        }
        if (x < w && y < h) {
            const size_t o = VS_IDX((size_t)y * w + x, plane, 405);     // (+ 4 planes: inside the frame's coef_fs floats)
            out[o] = hx * pc.ig11;
            out[plane + o] = hy * pc.ig11;
            out[2 * plane + o] = (h0 * pc.ig03 + hxx * pc.ig33) + hyy * pc.ig34;
            out[3 * plane + o] = (h0 * pc.ig03 + hyy * pc.ig33) + hxx * pc.ig34;
            out[4 * plane + o] = hxy * pc.ig55;
        }
    }
}

// ---- matrix update --------------------------------------------------------------------------------------------------------
// pair p = frames (p, p + 1) of the chunk; R0 / R1 their coefficient planes, M the pair's 5 output planes
__device__ __forceinline__ void update_px(const float* __restrict__ R0, const float* __restrict__ R1, size_t plane, int w, int h, int x, int y,
                                          float dx, float dy, float* __restrict__ M) {
    const float fx = fminf(fmaxf((float)x + dx, 0.0f), (float)(w - 1));
    const float fy = fminf(fmaxf((float)y + dy, 0.0f), (float)(h - 1));
    const int x0 = (int)fx, y0 = (int)fy;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const size_t i00 = VS_IDX((size_t)y0 * w + x0, plane, 406), i10 = VS_IDX((size_t)y0 * w + x1, plane, 406);
    const size_t i01 = VS_IDX((size_t)y1 * w + x0, plane, 406), i11 = VS_IDX((size_t)y1 * w + x1, plane, 406);
    float s[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const float* P = R1 + c * plane;
        s[c] = bilerp(P[i00], P[i10], P[i01], P[i11], tx, ty);
    }
    const size_t o = VS_IDX((size_t)y * w + x, plane, 407);            // R0's and M's five planes
    const float a11 = (R0[2 * plane + o] + s[2]) * 0.5f;
    const float a22 = (R0[3 * plane + o] + s[3]) * 0.5f;
    const float a12 = (R0[4 * plane + o] + s[4]) * 0.5f;
    const float bx = (R0[o] - s[0]) * 0.5f + (a11 * dx + a12 * dy);
    const float by = (R0[plane + o] - s[1]) * 0.5f + (a12 * dx + a22 * dy);
    M[o] = a11 * a11 + a12 * a12;
    M[plane + o] = a11 * a12 + a12 * a22;
    M[2 * plane + o] = a12 * a12 + a22 * a22;
    M[3 * plane + o] = a11 * bx + a12 * by;
    M[4 * plane + o] = a12 * bx + a22 * by;
}

// first update of a layer: the coarser layer's flow (dense float2 wc x hc per pair, or none on the top layer) resampled
__global__ __launch_bounds__(kThreads) void vs_k_flow_update_first(const float* __restrict__ coef, size_t coef_fs, int w, int h,
                                                                   const float2* __restrict__ Fc, size_t fc_ps, int wc, int hc, float rx, float ry,
                                                                   float inv_scale, float* __restrict__ M, size_t m_ps) {
    const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y, p = blockIdx.z;
    if (x >= w) return;
    float dx = 0.0f, dy = 0.0f;
    if (Fc) {
        const float2* F = Fc + p * fc_ps;
        int x0, x1, y0, y1;
        float tx, ty;
        src_coord(x, rx, wc, x0, x1, tx);
        src_coord(y, ry, hc, y0, y1, ty);
        const size_t nc = (size_t)wc * hc;
        (void)nc;
        const float2 f00 = F[VS_IDX((size_t)y0 * wc + x0, nc, 408)], f10 = F[VS_IDX((size_t)y0 * wc + x1, nc, 408)];
        const float2 f01 = F[VS_IDX((size_t)y1 * wc + x0, nc, 408)], f11 = F[VS_IDX((size_t)y1 * wc + x1, nc, 408)];
        dx = bilerp(f00.x, f10.x, f01.x, f11.x, tx, ty) * inv_scale;
        dy = bilerp(f00.y, f10.y, f01.y, f11.y, tx, ty) * inv_scale;
    }
    update_px(coef + p * coef_fs, coef + (p + 1) * coef_fs, (size_t)w * h, w, h, x, y, dx, dy, M + p * m_ps);
}

// ---- box blur + solve (+ next update | final outputs) ------------------------------------------------------------------------
// One 64 x 16 tile per workgroup; each of the five planes in turn: tile + halo into LDS, vertical box sums, horizontal box sums.
// Mn != null: the next update at the solved flow into Mn.  Otherwise the layer's result: flow (float2 at fo + y*fstride/2 + x,
// fstride in floats) and / or the squared magnitude (mag2, dense per pair).
constexpr int kBoxPitch = kTW + kMaxWin - 1;                    // 94 floats
constexpr int kBoxTile = (kTH + kMaxWin - 1) * kBoxPitch, kBoxVs = kTH * kBoxPitch;
__global__ __launch_bounds__(kThreads) void vs_k_flow_blur_solve(const float* __restrict__ M, size_t m_ps, int w, int h, int win,
                                                                 const float* __restrict__ coef, size_t coef_fs, float* __restrict__ Mn,
                                                                 float* __restrict__ fo, size_t fo_ps, int fstride, float* __restrict__ mag2,
                                                                 size_t mag_ps) {
    __shared__ float tile[kBoxTile];
    __shared__ float vs[kBoxVs];
    const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH, tid = threadIdx.x, p = blockIdx.z;
    const int lo = -(win / 2), cols = kTW + win - 1, rows = kTH + win - 1;
    const size_t plane = (size_t)w * h;
    const float* Mp = M + p * m_ps;
    constexpr int kPer = kTH / (kThreads / kTW);                 // 4 outputs per thread
    float m[5][kPer];
    const int c = tid % kTW;
    for (int q = 0; q < 5; q++) {
        const float* P = Mp + q * plane;
        for (int i = tid; i < rows * cols; i += kThreads) {
            const int r = i / cols, cc = i - r * cols;
            tile[VS_IDX(r * kBoxPitch + cc, kBoxTile, 409)] = P[VS_IDX((size_t)clampi(y0 + lo + r, 0, h - 1) * w + clampi(x0 + lo + cc, 0, w - 1), plane, 410)];
        }
        __syncthreads();
        for (int i = tid; i < kTH * cols; i += kThreads) {
            const int r = i / cols, cc = i - r * cols;
            float s = 0.0f;
            for (int t = 0; t < win; t++) s = s + tile[VS_IDX((r + t) * kBoxPitch + cc, kBoxTile, 411)];
            vs[VS_IDX(r * kBoxPitch + cc, kBoxVs, 412)] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            const int r = tid / kTW + j * (kThreads / kTW);
            float s = 0.0f;
            for (int t = 0; t < win; t++) s = s + vs[VS_IDX(r * kBoxPitch + c + t, kBoxVs, 413)];
            m[q][j] = s;
        }
        __syncthreads();
    }
    const int x = x0 + c;
    if (x >= w) return;
#pragma unroll
    for (int j = 0; j < kPer; j++) {
        const int y = y0 + tid / kTW + j * (kThreads / kTW);
        if (y >= h) continue;
        const float det = m[0][j] * m[2][j] - m[1][j] * m[1][j];
        const float idet = 1.0f / (fmaxf(det, 0.0f) + 1e-3f);
        const float dx = (m[2][j] * m[3][j] - m[1][j] * m[4][j]) * idet;
        const float dy = (m[0][j] * m[4][j] - m[1][j] * m[3][j]) * idet;
        if (Mn) {
            update_px(coef + p * coef_fs, coef + (p + 1) * coef_fs, plane, w, h, x, y, dx, dy, Mn + p * m_ps);
        } else {
            if (fo) {
                float* f = fo + p * fo_ps + VS_IDX((size_t)y * fstride + 2 * x, (size_t)(h - 1) * fstride + 2 * (size_t)w - 1, 420);
                f[0] = dx;
                f[1] = dy;
            }
            if (mag2) mag2[p * mag_ps + VS_IDX((size_t)y * w + x, plane, 414)] = dx * dx + dy * dy;
        }
    }
}

// ---- exact selection of element k of the squared magnitudes (non-negative floats: the bit patterns order like the values) ----
// pass 0: bits 31..21, pass 1: bits 20..10, pass 2: bits 9..0, each among the values whose higher bits match the prefix so far
__device__ __forceinline__ void pass_geometry(int pass, int& shift, uint32_t& mask, int& bins) {
    shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    bins = pass == 2 ? 1024 : 2048;
    mask = pass == 0 ? 0u : (0xFFFFFFFFu << (pass == 1 ? 21 : 10));
}
__global__ __launch_bounds__(kThreads) void vs_k_flow_hist(const uint32_t* __restrict__ bits, size_t ps, int n, int pass,
                                                           const SelState* __restrict__ st, uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[kHistBins];
    const int p = blockIdx.z;
    int shift, bins;
    uint32_t mask;
    pass_geometry(pass, shift, mask, bins);
    const uint32_t prefix = pass == 0 ? 0u : st[p].prefix;
    for (int i = threadIdx.x; i < kHistBins; i += kThreads) lh[i] = 0;
    __syncthreads();
    const uint32_t* b = bits + p * ps;
    for (int i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const uint32_t v = b[i];
        if ((v & mask) == prefix) atomicAdd(&lh[VS_IDX((v >> shift) & (uint32_t)(bins - 1), bins, 415)], 1u);
    }
    __syncthreads();
    uint32_t* g = hist + ((size_t)pass * gridDim.z + p) * kHistBins;
    for (int i = threadIdx.x; i < bins; i += kThreads)
        if (lh[VS_IDX(i, kHistBins, 416)]) atomicAdd(&g[VS_IDX(i, bins, 417)], lh[i]);
}
// one workgroup per pair: the bin that holds element k of the candidates; prefix and k move on to it
__global__ __launch_bounds__(kThreads) void vs_k_flow_pick(const uint32_t* __restrict__ hist, int pass, uint32_t k0, SelState* __restrict__ st) {
    constexpr int kPerT = kHistBins / kThreads;                  // 8 bins per thread
    __shared__ uint32_t sums[kThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    int shift, bins;
    uint32_t mask;
    pass_geometry(pass, shift, mask, bins);
    const uint32_t* g = hist + ((size_t)pass * gridDim.x + p) * kHistBins;
    uint32_t loc[kPerT];
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < kPerT; i++) { loc[i] = tid * kPerT + i < bins ? g[VS_IDX(tid * kPerT + i, bins, 418)] : 0u; s += loc[i]; }
    sums[VS_IDX(tid, kThreads, 419)] = s;
    const uint32_t k = pass == 0 ? k0 : st[p].k;
    const uint32_t prefix = pass == 0 ? 0u : st[p].prefix;
    __syncthreads();
    if (tid == 0) {                                              // exclusive prefix over the threads' sums
        uint32_t run = 0;
        for (int i = 0; i < kThreads; i++) { const uint32_t v = sums[i]; sums[i] = run; run += v; }
    }
    __syncthreads();
    uint32_t cum = sums[VS_IDX(tid, kThreads, 419)];
    if (cum <= k && k < cum + s) {                               // exactly one thread holds element k
        for (int i = 0; i < kPerT; i++) {
            if (k < cum + loc[i]) {
                st[p].prefix = prefix | ((uint32_t)(tid * kPerT + i) << shift);
                st[p].k = k - cum;
                break;
            }
            cum += loc[i];
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

std::vector<double> gauss_double(double sigma, int r) {             // tests/_flow_ref.py gauss_double
    std::vector<double> e((size_t)(2 * r + 1));
    double s = 0.0;
    for (int t = -r; t <= r; t++) { e[(size_t)(t + r)] = std::exp(-(double)(t * t) / (2.0 * sigma * sigma)); s += e[(size_t)(t + r)]; }
    for (double& v : e) v = v / s;
    return e;
}

struct Layer { int w, h; double scale; };
std::vector<Layer> layers_of(int w, int h, double pyr_scale, int levels) {
    std::vector<Layer> L;
    double s = 1.0;
    for (int k = 0; k <= levels; k++) {
        if (k) s *= pyr_scale;
        L.push_back({std::max(1, (int)std::floor(w * s + 0.5)), std::max(1, (int)std::floor(h * s + 0.5)), s});
    }
    return L;
}

bool pyr_radius(double scale, double& sigma, int& r) {
    sigma = (1.0 / scale - 1.0) * 0.5;
    const double rr = std::max(1.0, std::ceil(3.0 * sigma));
    if (!(rr <= kMaxPyrR)) return false;
    r = (int)rr;
    return true;
}

bool pyr_taps(double scale, PyrTaps& taps, int& r) {
    double sigma;
    if (!pyr_radius(scale, sigma, r)) return false;
    const std::vector<double> g = gauss_double(sigma, r);
    memset(&taps, 0, sizeof taps);
    for (int i = 0; i <= 2 * r; i++) taps.v[i] = (float)g[(size_t)i];
    return true;
}

PolyConsts poly_consts(int n, double sigma) {
    PolyConsts pc;
    memset(&pc, 0, sizeof pc);
    const std::vector<double> gd = gauss_double(sigma, n);
    double S0 = 0.0, S2 = 0.0, S4 = 0.0;
    for (int t = -n; t <= n; t++) {
        const double g = gd[(size_t)(t + n)];
        pc.g[t + n] = (float)g;
        pc.gt[t + n] = (float)(g * (double)t);
        pc.gtt[t + n] = (float)(g * (double)(t * t));
        S0 += g;
        S2 += g * (double)(t * t);
        S4 += g * (double)(t * t * t * t);
    }
    const double a = S0 * S0, b = S0 * S2, c = S0 * S4, d = S2 * S2;
    const double D1 = a * (c + d) - 2.0 * b * b;
    pc.ig11 = (float)(1.0 / (S2 * S0));
    pc.ig03 = (float)(-b / D1);
    pc.ig33 = (float)(0.5 * (a / D1 + 1.0 / (c - d)));
    pc.ig34 = (float)(0.5 * (a / D1 - 1.0 / (c - d)));
    pc.ig55 = (float)(0.5 / (S2 * S2));
    return pc;
}

}  // namespace

using vsi::set_error;
#define VSF_TRY(expr) do { int _r = (expr); if (_r != VS_OK) return _r; } while (0)
#define VSF_ARG(cond) do { if (!(cond)) return set_error(VS_ERR_ARG, "bad argument: %s (%s)", #cond, __func__); } while (0)

struct vs_flow {
    vs_flow_params p{};
    int device = 0;
    hipStream_t stream = nullptr;
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    ~vs_flow() {
        if (stream) (void)hipStreamSynchronize(stream);
        if (scratch) (void)hipFree(scratch);
        if (stream) (void)hipStreamDestroy(stream);
    }
    // grows the scratch to `bytes` (the contents are not kept); on failure the handle holds none and stays usable
    int reserve(size_t bytes) {
        if (bytes <= scratch_bytes) return VS_OK;
        if (scratch) {
            VS_HIP(hipStreamSynchronize(stream));
            (void)hipFree(scratch);
            scratch = nullptr;
            scratch_bytes = 0;
        }
        VS_HIP(vsi::dev_alloc(&scratch, bytes));
        scratch_bytes = bytes;
        return VS_OK;
    }
};

namespace {

// where the pieces of one chunk (C frames, C - 1 pairs, level-0 extent w x h) live inside the scratch
struct ChunkLayout {
    size_t N = 0;                          // level-0 pixels
    size_t gray = 0, V = 0, L = 0, coef = 0, M0 = 0, M1 = 0, FA = 0, FB = 0, mag = 0, hist = 0, st = 0, total = 0;
    static size_t frame_bytes(size_t N) { return align_up(N) + 2 * align_up(4 * N) + align_up(20 * N); }
    static size_t pair_bytes(size_t N) { return 2 * align_up(20 * N) + 2 * align_up(8 * N) + align_up(4 * N) + 3 * kHistBins * 4 + 8; }
    void make(size_t n_px, int C) {
        N = n_px;
        const size_t P = (size_t)(C - 1);
        size_t o = 0;
        gray = o; o += (size_t)C * align_up(N);
        V = o; o += (size_t)C * align_up(4 * N);
        L = o; o += (size_t)C * align_up(4 * N);
        coef = o; o += (size_t)C * align_up(20 * N);
        M0 = o; o += P * align_up(20 * N);
        M1 = o; o += P * align_up(20 * N);
        FA = o; o += P * align_up(8 * N);
        FB = o; o += P * align_up(8 * N);
        mag = o; o += P * align_up(4 * N);
        hist = o; o += align_up(3 * P * kHistBins * 4);
        st = o; o += align_up(P * sizeof(SelState));
        total = o;
    }
};

int chunk_frames(size_t N, int n) {
    const size_t fb = ChunkLayout::frame_bytes(N), pb = ChunkLayout::pair_bytes(N);
    const size_t c = (kMemCap + pb) / (fb + pb);
    return (int)std::max<size_t>(2, std::min<size_t>(c, (size_t)n));
}

int check_params(const vs_flow_params& p) {
    if (p.flags != 0) return set_error(VS_ERR_UNSUPPORTED, "vs_flow: flags %d (only 0: box window, no initial flow)", p.flags);
    if (!(p.pyr_scale > 0.0 && p.pyr_scale < 1.0) || p.levels < 0 || p.levels > 15 || p.winsize < 1 || p.winsize > kMaxWin ||
        p.iterations < 1 || p.iterations > 100 || p.poly_n < 1 || p.poly_n > kMaxPolyN || !(p.poly_sigma > 0.0))
        return set_error(VS_ERR_ARG, "vs_flow: parameters out of range (0 < pyr_scale < 1, levels 0..15, winsize 1..%d, iterations 1..100, "
                                     "poly_n 1..%d, poly_sigma > 0)", kMaxWin, kMaxPolyN);
    return VS_OK;
}

// Parameters in range can still ask for a pyramid blur the kernels do not have (sigma grows as 1/scale): refused per call, on the
// host, before anything of the call is allocated, copied or launched.
int check_layers(const vs_flow_params& p, int w, int h) {
    const std::vector<Layer> lay = layers_of(w, h, p.pyr_scale, p.levels);
    for (int k = 1; k <= p.levels; k++) {
        double sigma;
        int r = 0;
        if (!pyr_radius(lay[(size_t)k].scale, sigma, r))
            return set_error(VS_ERR_UNSUPPORTED, "vs_flow: layer %d needs a pyramid blur wider than %d taps", k, 2 * kMaxPyrR + 1);
    }
    return VS_OK;
}

// The flow of the C - 1 pairs of a chunk whose gray frames are in the layout's `gray` slots (dense, stride w).  Layer 0's result
// goes to `flow_out` (per pair fo_ps floats apart, row stride fstride floats) and / or the squared magnitudes to the `mag` slots.
int run_chunk(vs_flow* f, const ChunkLayout& Lo, int C, int w, int h, float* flow_out, size_t fo_ps, int fstride, bool want_mag) {
    const vs_flow_params& p = f->p;
    hipStream_t s = f->stream;
    char* base = (char*)f->scratch;
    const size_t N = Lo.N, gfs = align_up(N), ffs = align_up(4 * N) / 4, cfs = align_up(20 * N) / 4, mps = cfs, fps = align_up(8 * N) / 8;
    const uint8_t* gray = (const uint8_t*)(base + Lo.gray);
    float* V = (float*)(base + Lo.V);
    float* Lk = (float*)(base + Lo.L);
    float* coef = (float*)(base + Lo.coef);
    float* Mbuf[2] = {(float*)(base + Lo.M0), (float*)(base + Lo.M1)};
    float2* Fbuf[2] = {(float2*)(base + Lo.FA), (float2*)(base + Lo.FB)};
    const int P = C - 1;
    const std::vector<Layer> lay = layers_of(w, h, p.pyr_scale, p.levels);
    const PolyConsts pc = poly_consts(p.poly_n, p.poly_sigma);
    const float inv_scale = (float)(1.0 / p.pyr_scale);
    const float2* coarse = nullptr;
    int wc = 0, hc = 0;
    for (int k = p.levels; k >= 0; k--) {
        const int wk = lay[(size_t)k].w, hk = lay[(size_t)k].h;
        const dim3 tiles(cdiv(wk, kTW), cdiv(hk, kTH));
        if (k == 0) {
            vs_k_flow_polyexp<uint8_t><<<dim3(tiles.x, tiles.y, C), kThreads, 0, s>>>(gray, gfs, w, w, h, p.poly_n, pc, coef, cfs);
        } else {
            PyrTaps taps;
            int r = 0;
            if (!pyr_taps(lay[(size_t)k].scale, taps, r)) return set_error(VS_ERR_STATE, "vs_flow: layer %d was not checked", k);      // (check_layers)
            vs_k_flow_vblur<<<dim3(cdiv(w, kThreads), h, C), kThreads, 0, s>>>(gray, gfs, w, w, h, taps, r, V, ffs);
            vs_k_flow_hblur_resize<<<dim3(cdiv(wk, kThreads), hk, C), kThreads, 0, s>>>(V, ffs, w, h, taps, r, (float)((double)w / wk),
                                                                                      (float)((double)h / hk), Lk, ffs, wk, hk);
            vs_k_flow_polyexp<float><<<dim3(tiles.x, tiles.y, C), kThreads, 0, s>>>(Lk, ffs, wk, wk, hk, p.poly_n, pc, coef, cfs);
        }
        vs_k_flow_update_first<<<dim3(cdiv(wk, kThreads), hk, P), kThreads, 0, s>>>(
            coef, cfs, wk, hk, coarse, fps, wc, hc, coarse ? (float)((double)wc / wk) : 0.0f, coarse ? (float)((double)hc / hk) : 0.0f,
            inv_scale, Mbuf[0], mps);
        int cur = 0;
        float2* fine = Fbuf[k & 1];
        for (int it = 0; it < p.iterations; it++) {
            const bool last = it + 1 == p.iterations;
            float* fo = nullptr;
            size_t fo_stride_ps = 0;
            int fs = 0;
            float* mag = nullptr;
            if (last) {
                if (k > 0) { fo = (float*)fine; fo_stride_ps = 2 * fps; fs = 2 * wk; }
                else {
                    fo = flow_out; fo_stride_ps = fo_ps; fs = fstride;
                    if (want_mag) mag = (float*)(base + Lo.mag);
                }
            }
            vs_k_flow_blur_solve<<<dim3(tiles.x, tiles.y, P), kThreads, 0, s>>>(Mbuf[cur], mps, wk, hk, p.winsize, coef, cfs,
                                                                               last ? nullptr : Mbuf[cur ^ 1], fo, fo_stride_ps, fs, mag, ffs);
            cur ^= 1;
        }
        coarse = fine;
        wc = wk;
        hc = hk;
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// element n/2 of every pair's squared magnitudes -> out[P] (host), then the correctly rounded square root
int select_medians(vs_flow* f, const ChunkLayout& Lo, int P, int w, int h, float* out) {
    hipStream_t s = f->stream;
    char* base = (char*)f->scratch;
    const int n = w * h;
    const size_t ps = align_up(4 * Lo.N) / 4;
    uint32_t* hist = (uint32_t*)(base + Lo.hist);
    SelState* st = (SelState*)(base + Lo.st);
    VS_HIP(hipMemsetAsync(hist, 0, (size_t)3 * P * kHistBins * 4, s));
    const int blocks = std::max(1, std::min(cdiv(n, kThreads * 16), 256));
    for (int pass = 0; pass < 3; pass++) {
        vs_k_flow_hist<<<dim3(blocks, 1, P), kThreads, 0, s>>>((const uint32_t*)(base + Lo.mag), ps, n, pass, st, hist);
        vs_k_flow_pick<<<P, kThreads, 0, s>>>(hist, pass, (uint32_t)(n / 2), st);
    }
    VS_HIP(hipGetLastError());
    std::vector<SelState> h_st((size_t)P);
    VS_HIP(hipMemcpyAsync(h_st.data(), st, (size_t)P * sizeof(SelState), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < P; i++) {
        float v;
        memcpy(&v, &h_st[(size_t)i].prefix, sizeof v);
        out[i] = std::sqrt(v);
    }
    return VS_OK;
}

double median_of(std::vector<double> v) {                 // eval_jitter.cpp:8-19
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    const size_t n = v.size() / 2;
    return v.size() % 2 ? v[n] : 0.5 * (v[n] + v[n - 1]);
}

int enter(vs_flow* f) {
    if (!vsi::device_ready()) return VS_ERR_HIP;
    VS_HIP(hipSetDevice(f->device));
    return VS_OK;
}

}  // namespace

extern "C" {

void vs_flow_params_default(vs_flow_params* p) {
    if (!p) return;
    p->pyr_scale = 0.5;
    p->levels = 3;
    p->winsize = 15;
    p->iterations = 3;
    p->poly_n = 5;
    p->poly_sigma = 1.2;
    p->flags = 0;
}

vs_flow* vs_flow_create(const vs_flow_params* params, int device) try {
    if (!vsi::device_ready()) return nullptr;
    vs_flow_params p;
    if (params) p = *params; else vs_flow_params_default(&p);
    if (check_params(p) != VS_OK) return nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        set_error(VS_ERR_ARG, "device %d out of range (%d devices)", device, n);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error(VS_ERR_HIP, "hipSetDevice(%d) failed", device); return nullptr; }
    vs_flow* f = new vs_flow();
    f->p = p;
    f->device = device;
    if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) {
        f->stream = nullptr;
        delete f;
        set_error(VS_ERR_HIP, "hipStreamCreate failed");
        return nullptr;
    }
    return f;
} VS_CATCH_ALL_NULL

void vs_flow_destroy(vs_flow* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    delete f;
}

int vs_flow_compute(vs_flow* f, const uint8_t* prev, const uint8_t* next, int w, int h, int stride, int mem, float* flow,
                    int flow_stride) try {
    VSF_ARG(f && prev && next && flow && w > 0 && h > 0 && w <= 65535 && h <= 65535 && stride >= w && flow_stride >= 2 * w);
    VSF_ARG(mem == VS_MEM_HOST || mem == VS_MEM_DEVICE);
    VSF_TRY(check_layers(f->p, w, h));
    VSF_TRY(enter(f));
    hipStream_t s = f->stream;
    ChunkLayout Lo;
    Lo.make((size_t)w * h, 2);
    VSF_TRY(f->reserve(Lo.total));
    const size_t span = (size_t)(h - 1) * stride + w;
    vsi::Staged a, b, o;
    VSF_TRY(a.in(prev, span, mem, s));
    VSF_TRY(b.in(next, span, mem, s));
    VSF_TRY(o.out_image(flow, (size_t)2 * w * sizeof(float), (size_t)h, (size_t)flow_stride * sizeof(float), 1, 0, mem));
    uint8_t* gray = (uint8_t*)f->scratch + Lo.gray;
    VS_HIP(hipMemcpy2DAsync(gray, w, a.dev, stride, w, h, hipMemcpyDeviceToDevice, s));
    VS_HIP(hipMemcpy2DAsync(gray + align_up(Lo.N), w, b.dev, stride, w, h, hipMemcpyDeviceToDevice, s));
    VSF_TRY(run_chunk(f, Lo, 2, w, h, o.as<float>(), 0, flow_stride, false));
    VSF_TRY(o.finish(s));
    VS_HIP(hipStreamSynchronize(s));           // always: the handle's stream is not the caller's
    vsi::host_synced();
    o.complete();
    return VS_OK;
} VS_CATCH_ALL

int vs_flow_jitter(vs_flow* f, const void* frames, size_t frame_stride, int n, int w, int h, int stride, int format, int mem,
                   float* pair_medians, double* median) try {
    VSF_ARG(f && frames && pair_medians && median && n >= 2 && w > 0 && h > 0 && w <= 65535 && h <= 65535 && (long long)w * h < (1LL << 31));
    VSF_ARG(mem == VS_MEM_HOST || mem == VS_MEM_DEVICE);
    const int bits = vs_format_bits(format);
    if (bits == 0) return set_error(VS_ERR_ARG, "vs_flow_jitter: unknown format %d", format);
    const int ch = format == VS_FMT_GRAY8 ? 1 : 3;
    const size_t esz = bits > 8 ? 2 : 1;
    VSF_ARG(stride >= w * ch && frame_stride >= (size_t)(h - 1) * stride + (size_t)w * ch);
    VSF_TRY(check_layers(f->p, w, h));
    VSF_TRY(enter(f));
    hipStream_t s = f->stream;
    const size_t N = (size_t)w * h;
    const int C = chunk_frames(N, n);
    ChunkLayout Lo;
    Lo.make(N, C);
    VSF_TRY(f->reserve(Lo.total));
    const size_t span = (size_t)(h - 1) * stride + (size_t)w * ch;
    for (int f0 = 0; f0 + 1 < n; f0 += C - 1) {
        const int c = std::min(C, n - f0);
        vsi::Staged in;
        VSF_TRY(in.in((const char*)frames + (size_t)f0 * frame_stride * esz, ((size_t)(c - 1) * frame_stride + span) * esz, mem, s));
        uint8_t* gray = (uint8_t*)f->scratch + Lo.gray;
        if (ch == 1) {
            for (int i = 0; i < c; i++)
                VS_HIP(hipMemcpy2DAsync(gray + (size_t)i * align_up(N), w, (const uint8_t*)in.dev + (size_t)i * frame_stride, stride, w, h,
                                        hipMemcpyDeviceToDevice, s));
        } else {
            VS_HIP(vsk::bgr_to_gray(in.dev, w, h, stride, bits == 8 ? 8 : 16, bits - 8, gray, w, c, frame_stride, align_up(N), s));
        }
        VSF_TRY(run_chunk(f, Lo, c, w, h, nullptr, 0, 0, true));
        VSF_TRY(select_medians(f, Lo, c - 1, w, h, pair_medians + f0));
        vsi::host_synced();
    }
    std::vector<double> v((size_t)(n - 1));
    for (int i = 0; i + 1 < n; i++) v[(size_t)i] = pair_medians[i];
    *median = median_of(v);
    return VS_OK;
} VS_CATCH_ALL

}  // extern "C"

VS_BOUNDS_TU(vs_bounds_fetch_flow)
