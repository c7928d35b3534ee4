// vs_ycbcr.hip -- YCbCr frames to interleaved BGR and back (include/vs_amd.h: vs_ycbcr_to_bgr_batch, vs_bgr_to_ycbcr_batch; the rule:
// vs_ycbcr.hpp).  A pass of its own, in front of and behind everything: no other kernel file is touched.
//
// Both directions are streaming kernels with no reuse beyond a chroma cell: no LDS, no barrier, no scratch.  One descriptor serves every
// layout (planar or interleaved chroma, 4:2:0 / 4:2:2 / 4:4:4, luma only), so what differs between layouts is which loads a lane issues.
//
// WIDE FORM.  A lane owns 4 columns by `by` rows (by = 1 << sub_y: the rows of one chroma cell row); a wave a strip of 256 columns, a
// workgroup four cell rows; frames go in gridDim.y, chunked at 65535.  To BGR a lane loads, per row, one Y dword (8-bit) or dwordx2
// (16-bit), and once per cell row its chroma: planar 4:2:0 / 4:2:2 two samples per plane, planar 4:4:4 a dword (dwordx2) per plane,
// interleaved one run of Cb / Cr pairs; it stores three or six dwords per row.  To YCbCr is the mirror image: three or six dwords in per
// row, a Y dword (dwordx2) out per row and the chroma samples once per cell.  Taken when w % 4 == 0 and every row of every plane and of
// the BGR side starts on a dword.
//
// NARROW FORM.  One chroma cell per lane (bx x by pixels), element by element: any size, pitch and alignment, and the clamped right and
// bottom edges of odd frames (at an odd w the last cell holds one real column, whose values count twice in the average).  The same bits.
//
// Registers, occupancy and how the kernels stand against a plain copy: DESIGN.md "YCbCr frames".
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"
#include "vs_ycbcr.hpp"

using namespace vsd;

namespace {

constexpr int YC_W = 64, YC_WAVES = 4;        // a wave's strip is 64 lanes wide; four cell rows stacked make a workgroup's tile

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every row, column and frame offset of this file, sites 602-615.  To BGR: 602 / 603
// a Y row and column, 604 / 605 a chroma row and column (in elements of the run), 606 / 607 the BGR store's row and column, 608 the frame.
// To YCbCr: 609 / 610 the BGR load's row and column, 611 / 612 the Y store, 613 / 614 the chroma store, 615 the frame.  The extents are
// written inside the macros' arguments, which the regular build drops.

// the planes of a call as a kernel takes them: frame 0's first samples, strides in elements.  c: the first element of a chroma row's run
// (planar: the Cb plane, c2 the Cr plane; interleaved: the lower of the two pointers, cb_at: where Cb sits in a pair, 0 or 1)
template <typename T>
struct Planes {
    T* y; T* c; T* c2;
    int y_stride, c_stride, c_step, sub_x, sub_y, cb_at;
    size_t y_fs, c_fs;
};

// E elements of T as they lie in memory, in dwords (E * sizeof(T) is 2, or a multiple of 4 on a dword boundary)
template <int ND> struct __attribute__((packed, aligned(4))) yc_dw { uint32_t v[ND]; };
template <typename T, int E>
struct Run {
    static constexpr int BYTES = E * (int)sizeof(T), ND = BYTES >= 4 ? BYTES / 4 : 1;
    uint32_t v[ND];
    __device__ __forceinline__ void load(const T* p) {
        if constexpr (BYTES == 2) v[0] = *(const uint16_t*)p;
        else { const yc_dw<ND> q = *(const yc_dw<ND>*)p;
#pragma unroll
               for (int k = 0; k < ND; k++) v[k] = q.v[k]; }
    }
    __device__ __forceinline__ void store(T* p) const {
        if constexpr (BYTES == 2) *(uint16_t*)p = (uint16_t)v[0];
        else { yc_dw<ND> q;
#pragma unroll
               for (int k = 0; k < ND; k++) q.v[k] = v[k];
               *(yc_dw<ND>*)p = q; }
    }
    __device__ __forceinline__ int get(int k) const {
        return (int)px_get<T>(v, k);
    }
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int k = 0; k < ND; k++) v[k] = 0;
    }
    __device__ __forceinline__ void put(int k, int s) {        // (after clear(); s inside T's range)
        px_put<T>(v, k, (uint32_t)s);
    }
};

// ---- the wide form: SX = sub_x, CS = c_step -----------------------------------------------------------------------------------------
template <typename T, int SX, int CS>
__global__ __launch_bounds__(64 * YC_WAVES) void vs_k_ycbcr_to_bgr_wide(Planes<const T> p, int n, int w, int h, int sh, int maxv, T* __restrict__ dst, size_t dst_fs,
                                                                        int dst_stride, int tiles_x) {
    constexpr int NC = 4 >> SX;                                           // chroma cells of a lane's four columns
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x = 4 * (txi * YC_W + lane), cy = tyi * YC_WAVES + wv;
    const int ch = (h + p.sub_y) >> p.sub_y;
    if (cy >= ch || x >= w) return;                                       // (w is a multiple of 4: a lane's group is inside the row or past it)
    const size_t f = VS_IDX((size_t)blockIdx.y, n, 608);
    int cb[NC], cr[NC];
    if (p.c) {
        const size_t crow = f * p.c_fs + VS_IDX((size_t)cy * (size_t)p.c_stride, (long long)(ch - 1) * p.c_stride + 1, 604);
        const int ccol = VS_IDX((x >> SX) * CS, (long long)(w >> SX) * CS - (NC * CS - 1), 605);
        if (CS == 2) {
            Run<T, 2 * NC> u; u.load(p.c + crow + ccol);
#pragma unroll
            for (int k = 0; k < NC; k++) {                                // (selects, not a run-time index: the run stays in registers)
                const int a = u.get(2 * k), b = u.get(2 * k + 1);
                cb[k] = p.cb_at ? b : a; cr[k] = p.cb_at ? a : b;
            }
        } else {
            Run<T, NC> u, v; u.load(p.c + crow + ccol); v.load(p.c2 + crow + ccol);
#pragma unroll
            for (int k = 0; k < NC; k++) { cb[k] = u.get(k); cr[k] = v.get(k); }
        }
    } else {
#pragma unroll
        for (int k = 0; k < NC; k++) cb[k] = cr[k] = 128 << sh;
    }
    const int y0 = cy << p.sub_y, y1 = min(y0 + (1 << p.sub_y), h);
    for (int y = y0; y < y1; y++) {
        Run<T, 4> yy;
        yy.load(p.y + f * p.y_fs + VS_IDX((size_t)y * (size_t)p.y_stride, (long long)(h - 1) * p.y_stride + 1, 602) + VS_IDX(x, (long long)w - 3, 603));
        Run<T, 12> o; o.clear();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int b, g, r;
            vsy::to_bgr(yy.get(i), cb[i >> SX], cr[i >> SX], sh, maxv, b, g, r);
            o.put(3 * i, b); o.put(3 * i + 1, g); o.put(3 * i + 2, r);
        }
        o.store(dst + f * dst_fs + VS_IDX((size_t)y * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 606) + VS_IDX((size_t)x * 3, 3LL * w - 11, 607));
    }
}

template <typename T, int SX, int CS>
__global__ __launch_bounds__(64 * YC_WAVES) void vs_k_bgr_to_ycbcr_wide(const T* __restrict__ src, size_t src_fs, int src_stride, int n, int w, int h, int sh, int maxv,
                                                                        Planes<T> p, int tiles_x) {
    constexpr int NC = 4 >> SX;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x = 4 * (txi * YC_W + lane), cy = tyi * YC_WAVES + wv;
    const int ch = (h + p.sub_y) >> p.sub_y;
    if (cy >= ch || x >= w) return;
    const size_t f = VS_IDX((size_t)blockIdx.y, n, 615);
    int su[NC], sv[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) su[k] = sv[k] = 0;
    const int y0 = cy << p.sub_y, by = 1 << p.sub_y;
    for (int dy = 0; dy < by; dy++) {
        const int y = min(y0 + dy, h - 1);                                // (an odd h: the last cell row's one real row counts twice)
        Run<T, 12> in;
        in.load(src + f * src_fs + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 609) + VS_IDX((size_t)x * 3, 3LL * w - 11, 610));
        Run<T, 4> yy; yy.clear();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int l, cb, cr;
            vsy::to_ycbcr(in.get(3 * i), in.get(3 * i + 1), in.get(3 * i + 2), sh, maxv, l, cb, cr);
            yy.put(i, l);
            su[i >> SX] += cb; sv[i >> SX] += cr;
        }
        if (y0 + dy < h)
            yy.store(p.y + f * p.y_fs + VS_IDX((size_t)y * (size_t)p.y_stride, (long long)(h - 1) * p.y_stride + 1, 611) + VS_IDX(x, (long long)w - 3, 612));
    }
    if (!p.c) return;
    const size_t crow = f * p.c_fs + VS_IDX((size_t)cy * (size_t)p.c_stride, (long long)(ch - 1) * p.c_stride + 1, 613);
    const int ccol = VS_IDX((x >> SX) * CS, (long long)(w >> SX) * CS - (NC * CS - 1), 614);
    if (CS == 2) {
        Run<T, 2 * NC> u; u.clear();
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const int a = vsy::cell_average(su[k], SX, p.sub_y), b = vsy::cell_average(sv[k], SX, p.sub_y);
            u.put(2 * k, p.cb_at ? b : a); u.put(2 * k + 1, p.cb_at ? a : b);
        }
        u.store(p.c + crow + ccol);
    } else {
        Run<T, NC> u, v; u.clear(); v.clear();
#pragma unroll
        for (int k = 0; k < NC; k++) { u.put(k, vsy::cell_average(su[k], SX, p.sub_y)); v.put(k, vsy::cell_average(sv[k], SX, p.sub_y)); }
        u.store(p.c + crow + ccol); v.store(p.c2 + crow + ccol);
    }
}

// ---- the narrow form: one chroma cell per lane, element by element ---------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64 * YC_WAVES) void vs_k_ycbcr_to_bgr_narrow(Planes<const T> p, int n, int w, int h, int sh, int maxv, T* __restrict__ dst, size_t dst_fs,
                                                                          int dst_stride, int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int cx = txi * YC_W + lane, cy = tyi * YC_WAVES + wv;
    const int cw = (w + p.sub_x) >> p.sub_x, ch = (h + p.sub_y) >> p.sub_y;
    if (cy >= ch || cx >= cw) return;
    const size_t f = VS_IDX((size_t)blockIdx.y, n, 608);
    int cb = 128 << sh, cr = 128 << sh;
    if (p.c) {
        const size_t at = f * p.c_fs + VS_IDX((size_t)cy * (size_t)p.c_stride, (long long)(ch - 1) * p.c_stride + 1, 604) +
                          VS_IDX(cx * p.c_step, (long long)(cw - 1) * p.c_step + 1, 605);
        if (p.c_step == 2) { cb = p.c[at + p.cb_at]; cr = p.c[at + 1 - p.cb_at]; }
        else { cb = p.c[at]; cr = p.c2[at]; }
    }
    const int x0 = cx << p.sub_x, x1 = min(x0 + (1 << p.sub_x), w), y0 = cy << p.sub_y, y1 = min(y0 + (1 << p.sub_y), h);
    for (int y = y0; y < y1; y++)
        for (int x = x0; x < x1; x++) {
            const int l = p.y[f * p.y_fs + VS_IDX((size_t)y * (size_t)p.y_stride, (long long)(h - 1) * p.y_stride + 1, 602) + VS_IDX(x, w, 603)];
            int b, g, r;
            vsy::to_bgr(l, cb, cr, sh, maxv, b, g, r);
            T* const o = dst + f * dst_fs + VS_IDX((size_t)y * (size_t)dst_stride, (long long)(h - 1) * dst_stride + 1, 606) + VS_IDX((size_t)x * 3, 3LL * w - 2, 607);
            o[0] = (T)b; o[1] = (T)g; o[2] = (T)r;
        }
}

template <typename T>
__global__ __launch_bounds__(64 * YC_WAVES) void vs_k_bgr_to_ycbcr_narrow(const T* __restrict__ src, size_t src_fs, int src_stride, int n, int w, int h, int sh, int maxv,
                                                                          Planes<T> p, int tiles_x) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int cx = txi * YC_W + lane, cy = tyi * YC_WAVES + wv;
    const int cw = (w + p.sub_x) >> p.sub_x, ch = (h + p.sub_y) >> p.sub_y;
    if (cy >= ch || cx >= cw) return;
    const size_t f = VS_IDX((size_t)blockIdx.y, n, 615);
    const int bx = 1 << p.sub_x, by = 1 << p.sub_y;
    int su = 0, sv = 0;
    for (int dy = 0; dy < by; dy++)
        for (int dx = 0; dx < bx; dx++) {
            const int x = min(cx * bx + dx, w - 1), y = min(cy * by + dy, h - 1);       // the clamped right and bottom edges of odd frames
            const T* const s = src + f * src_fs + VS_IDX((size_t)y * (size_t)src_stride, (long long)(h - 1) * src_stride + 1, 609) + VS_IDX((size_t)x * 3, 3LL * w - 2, 610);
            int l, cb, cr;
            vsy::to_ycbcr(s[0], s[1], s[2], sh, maxv, l, cb, cr);
            if (cx * bx + dx < w && cy * by + dy < h)
                p.y[f * p.y_fs + VS_IDX((size_t)y * (size_t)p.y_stride, (long long)(h - 1) * p.y_stride + 1, 611) + VS_IDX(x, w, 612)] = (T)l;
            su += cb; sv += cr;
        }
    if (!p.c) return;
    const size_t at = f * p.c_fs + VS_IDX((size_t)cy * (size_t)p.c_stride, (long long)(ch - 1) * p.c_stride + 1, 613) +
                      VS_IDX(cx * p.c_step, (long long)(cw - 1) * p.c_step + 1, 614);
    const T u = (T)vsy::cell_average(su, p.sub_x, p.sub_y), v = (T)vsy::cell_average(sv, p.sub_x, p.sub_y);
    if (p.c_step == 2) { p.c[at + p.cb_at] = u; p.c[at + 1 - p.cb_at] = v; }
    else { p.c[at] = u; p.c2[at] = v; }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct Shape { bool ok; int sh; size_t esz; };
Shape shape_of(const vs_ycbcr_planes& pl, int n, int w, int h, int bits, int max_value) {
    Shape s{false, bits - 8, bits > 8 ? (size_t)2 : (size_t)1};
    if (bits < 8 || bits > 16 || max_value < 1 || max_value > (bits > 8 ? 65535 : 255)) return s;
    if (n < 1 || w < 1 || h < 1 || w > 32767 || h > 32767 || !vsy::layout_ok(pl, n, w, h)) return s;
    if (pl.cb && pl.c_step == 2 && (char*)pl.cb - (char*)pl.cr != (ptrdiff_t)s.esz && (char*)pl.cr - (char*)pl.cb != (ptrdiff_t)s.esz) return s;
    s.ok = true;
    return s;
}
template <typename P>
Planes<P> planes_of(const vs_ycbcr_planes& pl) {
    Planes<P> p{};
    p.y = (P*)pl.y;
    p.y_stride = pl.y_stride; p.c_stride = pl.c_stride; p.c_step = pl.c_step; p.sub_x = pl.sub_x; p.sub_y = pl.sub_y;
    p.y_fs = pl.y_frame_stride; p.c_fs = pl.c_frame_stride;
    if (pl.cb) {
        if (pl.c_step == 2) { p.cb_at = (uintptr_t)pl.cb < (uintptr_t)pl.cr ? 0 : 1; p.c = (P*)(p.cb_at ? pl.cr : pl.cb); p.c2 = nullptr; }
        else { p.c = (P*)pl.cb; p.c2 = (P*)pl.cr; }
    }
    return p;
}
// every row of every plane and of the BGR side starts on a dword, and w is a multiple of 4
bool wide_ok(const vs_ycbcr_planes& pl, int n, int w, size_t esz, const void* bgr, size_t bgr_fs, int bgr_stride) {
    bool ok = vsk::rows_on_dwords(bgr, bgr_stride, bgr_fs, n, esz) && vsk::rows_on_dwords(pl.y, pl.y_stride, pl.y_frame_stride, n, esz);
    if (pl.cb) {                                          // two planes, or one of pairs that starts at the lower of the two pointers
        if (pl.c_step == 1) ok = ok && vsk::rows_on_dwords(pl.cb, pl.c_stride, pl.c_frame_stride, n, esz) && vsk::rows_on_dwords(pl.cr, pl.c_stride, pl.c_frame_stride, n, esz);
        else ok = ok && vsk::rows_on_dwords((uintptr_t)pl.cb < (uintptr_t)pl.cr ? pl.cb : pl.cr, pl.c_stride, pl.c_frame_stride, n, esz);
    }
    return w % 4 == 0 && ok;
}
// frame f0's descriptor
vs_ycbcr_planes at_frame(vs_ycbcr_planes pl, size_t f0, size_t esz) {
    pl.y = (char*)pl.y + f0 * pl.y_frame_stride * esz;
    if (pl.cb) { pl.cb = (char*)pl.cb + f0 * pl.c_frame_stride * esz; pl.cr = (char*)pl.cr + f0 * pl.c_frame_stride * esz; }
    return pl;
}

template <typename T>
void launch_to_bgr(const vs_ycbcr_planes& pl, int n, int w, int h, int sh, int maxv, void* dst, size_t dst_fs, int dst_stride, bool wide, hipStream_t s) {
    const int cw = vsy::chroma_extent(w, pl.sub_x), ch = vsy::chroma_extent(h, pl.sub_y);
    const int tiles_x = ((wide ? w / 4 : cw) + YC_W - 1) / YC_W, tiles_y = (ch + YC_WAVES - 1) / YC_WAVES;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n), block(64 * YC_WAVES);
    const Planes<const T> p = planes_of<const T>(pl);
#define VS_YC_LAUNCH(SX, CS) hipLaunchKernelGGL((vs_k_ycbcr_to_bgr_wide<T, SX, CS>), grid, block, 0, s, p, n, w, h, sh, maxv, (T*)dst, dst_fs, dst_stride, tiles_x)
    if (!wide) hipLaunchKernelGGL((vs_k_ycbcr_to_bgr_narrow<T>), grid, block, 0, s, p, n, w, h, sh, maxv, (T*)dst, dst_fs, dst_stride, tiles_x);
    else if (pl.sub_x && pl.c_step == 2) VS_YC_LAUNCH(1, 2);
    else if (pl.sub_x) VS_YC_LAUNCH(1, 1);
    else if (pl.c_step == 2) VS_YC_LAUNCH(0, 2);
    else VS_YC_LAUNCH(0, 1);
#undef VS_YC_LAUNCH
}
template <typename T>
void launch_to_ycbcr(const void* src, size_t src_fs, int src_stride, int n, int w, int h, int sh, int maxv, const vs_ycbcr_planes& pl, bool wide, hipStream_t s) {
    const int cw = vsy::chroma_extent(w, pl.sub_x), ch = vsy::chroma_extent(h, pl.sub_y);
    const int tiles_x = ((wide ? w / 4 : cw) + YC_W - 1) / YC_W, tiles_y = (ch + YC_WAVES - 1) / YC_WAVES;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)n), block(64 * YC_WAVES);
    const Planes<T> p = planes_of<T>(pl);
#define VS_YC_LAUNCH(SX, CS) hipLaunchKernelGGL((vs_k_bgr_to_ycbcr_wide<T, SX, CS>), grid, block, 0, s, (const T*)src, src_fs, src_stride, n, w, h, sh, maxv, p, tiles_x)
    if (!wide) hipLaunchKernelGGL((vs_k_bgr_to_ycbcr_narrow<T>), grid, block, 0, s, (const T*)src, src_fs, src_stride, n, w, h, sh, maxv, p, tiles_x);
    else if (pl.sub_x && pl.c_step == 2) VS_YC_LAUNCH(1, 2);
    else if (pl.sub_x) VS_YC_LAUNCH(1, 1);
    else if (pl.c_step == 2) VS_YC_LAUNCH(0, 2);
    else VS_YC_LAUNCH(0, 1);
#undef VS_YC_LAUNCH
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_ycbcr)

namespace vsk {

hipError_t ycbcr_to_bgr(const vs_ycbcr_planes& src, int n_frames, int w, int h, int bits, int max_value, void* dst, size_t dst_fs, int dst_stride, hipStream_t s) {
    const Shape sp = shape_of(src, n_frames, w, h, bits, max_value);
    if (!sp.ok || !dst || dst_stride < 3 * w) return hipErrorNotSupported;
    const bool wide = wide_ok(src, n_frames, w, sp.esz, dst, dst_fs, dst_stride);
    vsk::for_frame_chunks(n_frames, [&](int f0, int nf) {
        char* const dp = (char*)dst + (size_t)f0 * dst_fs * sp.esz;
        if (sp.esz == 2) launch_to_bgr<uint16_t>(at_frame(src, (size_t)f0, sp.esz), nf, w, h, sp.sh, max_value, dp, dst_fs, dst_stride, wide, s);
        else launch_to_bgr<uint8_t>(at_frame(src, (size_t)f0, sp.esz), nf, w, h, sp.sh, max_value, dp, dst_fs, dst_stride, wide, s);
    });
    return hipGetLastError();
}

hipError_t bgr_to_ycbcr(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int bits, int max_value, const vs_ycbcr_planes& dst, hipStream_t s) {
    const Shape sp = shape_of(dst, n_frames, w, h, bits, max_value);
    if (!sp.ok || !src || src_stride < 3 * w) return hipErrorNotSupported;
    const bool wide = wide_ok(dst, n_frames, w, sp.esz, src, src_fs, src_stride);
    vsk::for_frame_chunks(n_frames, [&](int f0, int nf) {
        const char* const sp0 = (const char*)src + (size_t)f0 * src_fs * sp.esz;
        if (sp.esz == 2) launch_to_ycbcr<uint16_t>(sp0, src_fs, src_stride, nf, w, h, sp.sh, max_value, at_frame(dst, (size_t)f0, sp.esz), wide, s);
        else launch_to_ycbcr<uint8_t>(sp0, src_fs, src_stride, nf, w, h, sp.sh, max_value, at_frame(dst, (size_t)f0, sp.esz), wide, s);
    });
    return hipGetLastError();
}

}  // namespace vsk
