// vs_remap.hip -- remap of BGR frames through a map of fixed-point positions, and the radial lens map that the lens-distortion correction
// remaps with.  A lens bends the frame from inside in a way that is constant per clip, so the map is made once (vs_k_lens_map; the rule:
// vs_lens.hpp) and the remap forms positions, clamped tap offsets and weights once per pixel for all frames of a call.  A pass of its own:
// vs_warp.hip, vs_fill.hip and vs_rolling.hip are not touched.
//
// THE MAP FORMAT (also include/vs_amd.h).  A map for `ow x oh` output pixels is `int32_t` pairs `(X, Y)`.
//
// - Pixel `(u, v)` is at `map[v * map_stride + 2 * u]` and `+ 1`.
// - `map_stride` is in `int32_t` elements and is `>= 2 * ow`.
// - `X` and `Y` are source positions with 5 fraction bits: exactly what `vsd::cv_pos` produces (`CvPos`).
// - Every int32 value is legal.
//
// THE SAMPLE RULE (also include/vs_amd.h, vs_bgr_remap_batch; DESIGN.md "Lens-distortion correction").  Interleaved BGR, every `VS_FMT_BGR*`;
// `w, h, ow, oh` in 1 .. 32767, `VS_ERR_UNSUPPORTED` beyond, as the rolling-shutter pass does.
//
// - Taps sit at `(X >> 5, Y >> 5)` and the three neighbours to the right and below. Fractions are `X & 31`, `Y & 31`.
// - The blend is `VS_WARP_BILINEAR_CV`'s (`cv_blend` in `vs_cv_sample.hpp`).
//   - 8-bit containers: integer weights, `(sum + 512) >> 10`.
//   - 16-bit containers: fp32 weights `a * b / 1024`, `rintf`, saturated to `vs_format_max_value(format)`.
// - `VS_BORDER_CLAMP`: each tap's column is clamped to `0 .. w - 1` and its row to `0 .. h - 1`, with weights unchanged. This is the
//   rolling-shutter pass's rule.
// - `VS_BORDER_CONSTANT`: a tap outside the frame counts as 0, with weights unchanged. This is `VS_WARP_BILINEAR_CV`'s rule under that border.
// - Tap index sums are taken so that no int32 `X` or `Y` overflows (`X >> 5` is below 2^26).
//
// Hence
//
// - (a) The map `X = 32 u, Y = 32 v` with `ow == w, oh == h` returns every frame bit for bit. This holds for samples up to the format's maximum.
// - (b) Under the clamp border, every output sample lies between the minimum and maximum of the frame's samples in its channel.
// - (c) Every sample is defined for every map.
//
// KERNEL.  vs_k_bgr_rolling's shape: a wave owns a strip of 64 (PX = 1) or 256 (PX = 4) columns and walks 8 rows; no LDS, no barrier, no
// scratch; a row's two taps come as ONE unaligned load of eight elements pulled back from the row's end (WIDE: w >= 3); PX = 4 lanes store three
// or six dwords (ow a multiple of 4, destination rows on dwords).  What is new: a lane reads its positions as a dwordx2 per pixel from the map
// and forms, ONCE, the two clamped load offsets, the shift that puts tap c0 at the bottom, and the four weight products -- an outside tap of
// the constant border gets the weight 0, which is that tap counting as 0: v * 0 is 0 in the int32 sum, and (float)v * 0.0f is +0.0f, what
// 0.0f * w is, in the fp32 one.  Then it loops over a slice of the call's frames (gridDim.y = ceil(n / slice)): per frame and pixel only the
// two loads, the unpack, the blend and the store remain.  Slice length, registers and occupancy of each instantiation, and what the map's
// bytes cost: DESIGN.md "Lens-distortion correction".
#include <algorithm>

#include "vs_kernels.hpp"
#include "vs_device.hpp"
#include "vs_cv_sample.hpp"
#include "vs_launch.hpp"
#include "vs_lens.hpp"

using namespace vsd;

namespace {

constexpr int RM_W = 64, RM_WAVES = 4, RM_ROWS = 8;       // a wave's strip is 64 lanes wide and 8 rows high; four strips stacked make a workgroup's tile

// The bounds build (-DVS_DEBUG_BOUNDS, vs_device.hpp) checks every map read, every gather and every store of this file, sites 591-601: 591 / 592
// a map entry's row and column offsets; 593 / 594 a gather's two row offsets, 595 / 596 its column offsets; 597 the frame of the slice; 598 / 599
// the store's row and column offsets; 600 / 601 the lens map's store.  The extents are written inside the macros' arguments, which the regular
// build drops.

struct __attribute__((packed, aligned(4))) rm_pos { int32_t X, Y; };                  // a map entry: a dwordx2 on a dword boundary

// What a pixel keeps across the frames of a slice.  o0, o1: element offsets, from the frame's first sample, of the loads of rows sy and sy + 1
// (WIDE: the start of the eight-element load, pulled back from the row's end so that every byte read lies inside the row; else tap c0's first
// sample); sh: WIDE, the bits that put tap c0 at the bottom; d1: the second tap's distance from the first in samples, 3 or (the clamp folded
// them) 0; wt: the four weight products a0 b0, a1 b0, a0 b1, a1 b1 (8-bit containers: int; 16-bit: the products times 1 / 1024 in fp32).
// The loads and their unpacking are vs_cv_sample.hpp's row_fetch and row_unpack, used apart: a lane has the loads of all its pixels in flight
// before it unpacks the first (with a load and its unpack back to back the kernel waited out a memory latency per frame row).
template <typename T>
struct Plan {
    long long o0, o1;
    int sh, d1;
    typename Weight<T>::type wt[4];
};

template <typename T, bool WIDE>
__device__ __forceinline__ Plan<T> rm_plan(CvPos p, int w, int h, int stride, int border) {
    const int sx = p.X >> 5, sy = p.Y >> 5;              // (|sx|, |sy| <= 2^26: sx + 1 cannot overflow)
    const int c0 = clampi(sx, 0, w - 1), c1 = clampi(sx + 1, 0, w - 1), r0 = clampi(sy, 0, h - 1), r1 = clampi(sy + 1, 0, h - 1);
    Plan<T> pl;
    const int e0 = c0 * 3;
    int col;
    if (WIDE) {
        col = VS_IDX(min(e0, 3 * w - 8), 3LL * w - 7, 595);
        pl.sh = 8 * (int)sizeof(T) * (e0 - col);          // (0 .. 5 samples)
    } else {
        col = VS_IDX(e0, 3LL * w - 2, 595);
        (void)VS_IDX(c1 * 3, 3LL * w - 2, 596);
        pl.sh = 0;
    }
    pl.d1 = (c1 - c0) * 3;
    pl.o0 = (long long)VS_IDX((size_t)r0 * (size_t)stride, (long long)(h - 1) * stride + 1, 593) + col;
    pl.o1 = (long long)VS_IDX((size_t)r1 * (size_t)stride, (long long)(h - 1) * stride + 1, 594) + col;
    int m[4];
    cv_products(p, m);
    if (border != VS_BORDER_CLAMP) {                      // constant border: a tap outside the frame counts as 0
        const bool x0in = sx == c0, x1in = sx + 1 == c1, y0in = sy == r0, y1in = sy + 1 == r1;
        m[0] = x0in && y0in ? m[0] : 0; m[1] = x1in && y0in ? m[1] : 0; m[2] = x0in && y1in ? m[2] : 0; m[3] = x1in && y1in ? m[3] : 0;
    }
    cv_weights<T>(m, pl.wt);
    return pl;
}

// a frame's loads for a lane's PX pixels: rows sy and sy + 1 of each
template <typename T, int PX, bool WIDE>
__device__ __forceinline__ void rm_fetch_frame(GPtr<T> fs, const Plan<T> pl[PX], RowRaw<T, WIDE> raw[PX][2]) {
#pragma unroll
    for (int i = 0; i < PX; i++) {
        raw[i][0] = row_fetch(fs + pl[i].o0, pl[i].d1, (RowRaw<T, WIDE>*)nullptr);
        raw[i][1] = row_fetch(fs + pl[i].o1, pl[i].d1, (RowRaw<T, WIDE>*)nullptr);
    }
}
// a lane's PX pixels of one frame from what rm_fetch_frame brought: unpack, blend, store (PX == 4: three or six dwords)
template <typename T, int PX, bool WIDE>
__device__ __forceinline__ void rm_emit(const RowRaw<T, WIDE> raw[PX][2], const Plan<T> pl[PX], int maxv, T* op) {
    constexpr int ND = PX * 3 * (int)sizeof(T) / 4;                       // dwords of a lane's four pixels (PX == 4)
    uint32_t o[ND > 0 ? ND : 1];
#pragma unroll
    for (int k = 0; k < (ND > 0 ? ND : 1); k++) o[k] = 0;
#pragma unroll
    for (int i = 0; i < PX; i++) {
        uint32_t t[4][3], q[3];
        row_unpack(raw[i][0], pl[i].sh, pl[i].d1, t[0], t[1]);
        row_unpack(raw[i][1], pl[i].sh, pl[i].d1, t[2], t[3]);
        cv_blend(t, pl[i].wt, maxv, q);
        if (PX == 1) {
            op[0] = (T)q[0]; op[1] = (T)q[1]; op[2] = (T)q[2];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) px_put<T>(o, 3 * i + k, q[k]);
        }
    }
    if (PX > 1) {
#pragma unroll
        for (int k = 0; k < ND; k++) ((uint32_t*)op)[k] = o[k];
    }
}

// frames [blockIdx.y * slice, ...) of the call, at most `slice` of them.  PX: pixels per lane (1, or 4 with dword stores); WIDE: a row's two
// taps in one load (w >= 3)
template <typename T, int PX, bool WIDE>
__global__ __launch_bounds__(64 * RM_WAVES) void vs_k_bgr_remap(const T* __restrict__ src, size_t src_fs, int n, int slice, int w, int h, int src_stride,
                                                                int maxv, const int32_t* __restrict__ map, int map_stride, int ow, int oh, int border,
                                                                T* __restrict__ dst, size_t dst_fs, int dst_stride, int tiles_x) {
    constexpr int R = RM_ROWS;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tyi = (int)blockIdx.x / tiles_x, txi = (int)blockIdx.x - tyi * tiles_x;
    const int x = txi * PX * RM_W + PX * lane, y0 = (tyi * RM_WAVES + wv) * R;
    if (y0 >= oh || x >= ow) return;                                      // (PX == 4: ow is a multiple of 4, a lane's group is inside the row or past it)
    const int f0 = (int)blockIdx.y * slice, f1 = min(f0 + slice, n);
    const int y1 = min(y0 + R, oh);
    for (int v = y0; v < y1; v++) {
        const int32_t* const mrow = map + VS_IDX((size_t)v * (size_t)map_stride, (long long)(oh - 1) * map_stride + 1, 591);
        Plan<T> pl[PX];
        rm_pos mp[PX];
#pragma unroll
        for (int i = 0; i < PX; i++) mp[i] = *(const rm_pos*)(mrow + VS_IDX(2 * (x + i), 2LL * ow - 1, 592));
#pragma unroll
        for (int i = 0; i < PX; i++) pl[i] = rm_plan<T, WIDE>(CvPos{mp[i].X, mp[i].Y}, w, h, src_stride, border);
        const size_t oo = VS_IDX((size_t)v * (size_t)dst_stride, (long long)(oh - 1) * dst_stride + 1, 598) + VS_IDX((size_t)x * 3, 3LL * ow - (3 * PX - 1), 599);
        // A frame's loads go out as soon as the frame in front of it has been unpacked: they are in flight while that frame is blended and
        // stored.  Past the slice's end the last frame is fetched once more and not used: with a branch around the fetch the wait in front of
        // the unpack would wait for everything, stores included.  (Two sets of loads in turn, and two frames per iteration, took more registers
        // and no less time: DESIGN.md "Lens-distortion correction".)
        auto frame = [&](int f) { return (GPtr<T>)(src + (size_t)VS_IDX(min(f, f1 - 1), n, 597) * src_fs); };
        RowRaw<T, WIDE> raw[PX][2];
        rm_fetch_frame<T, PX, WIDE>(frame(f0), pl, raw);
        for (int f = f0; f < f1; f++) {
            rm_emit<T, PX, WIDE>(raw, pl, maxv, dst + (size_t)f * dst_fs + oo);
            rm_fetch_frame<T, PX, WIDE>(frame(f + 1), pl, raw);
        }
    }
}

// the radial map (the rule: vs_lens.hpp), one pixel per thread
__global__ __launch_bounds__(256) void vs_k_lens_map(vs_lens_params p, int w, int h, int32_t* __restrict__ map, int map_stride) {
    const int u = (int)(blockIdx.x * 64 + (threadIdx.x & 63)), v = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (u >= w || v >= h) return;
    int32_t X, Y;
    vsl::position(p, u, v, &X, &Y);
    int32_t* const o = map + VS_IDX((size_t)v * (size_t)map_stride, (long long)(h - 1) * map_stride + 1, 600) + VS_IDX(2 * u, 2LL * w - 1, 601);
    o[0] = X; o[1] = Y;
}

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_remap)

namespace vsk {

hipError_t bgr_remap(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int bits, int max_value, const int32_t* map,
                     int map_stride, int ow, int oh, int border, void* dst, size_t dst_fs, int dst_stride, int slice, hipStream_t s) {
    if (!container_ok(bits, max_value)) return hipErrorNotSupported;
    if (n_frames < 1 || w < 1 || h < 1 || w > 32767 || h > 32767 || ow < 1 || oh < 1 || ow > 32767 || oh > 32767 || slice < 1) return hipErrorNotSupported;
    if (border != VS_BORDER_CLAMP && border != VS_BORDER_CONSTANT) return hipErrorNotSupported;
    const size_t esz = (size_t)bits / 8;
    // four pixels per lane with dword stores where every destination row starts on a dword
    const bool x4 = ow % 4 == 0 && rows_on_dwords(dst, dst_stride, dst_fs, n_frames, esz);
    const int tw = x4 ? 4 * RM_W : RM_W, th = RM_ROWS * RM_WAVES;
    const int tiles_x = (ow + tw - 1) / tw, tiles_y = (oh + th - 1) / th;
    const int groups = (n_frames + slice - 1) / slice;
    for_frame_chunks(groups, [&](int g0, int ng) {         // (chunks of frame groups: gridDim.y counts slices)
        const size_t f0 = (size_t)g0 * slice;
        const int nf = (int)std::min<size_t>((size_t)n_frames - f0, (size_t)ng * slice);
        const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)ng), block(64 * RM_WAVES);
        const char* sp = (const char*)src + f0 * src_fs * esz;
        char* dp = (char*)dst + f0 * dst_fs * esz;
        // (the same arguments for every instantiation)
#define VS_RM_LAUNCH(T, PX, WIDE) hipLaunchKernelGGL((vs_k_bgr_remap<T, PX, WIDE>), grid, block, 0, s, (const T*)sp, src_fs, nf, slice, w, h, src_stride, max_value, map, map_stride, ow, oh, border, (T*)dp, dst_fs, dst_stride, tiles_x)
        if (w < 3) { if (bits == 16) VS_RM_LAUNCH(uint16_t, 1, false); else VS_RM_LAUNCH(uint8_t, 1, false); }      // (a row of fewer than eight elements)
        else if (x4 && bits == 16) VS_RM_LAUNCH(uint16_t, 4, true);
        else if (x4) VS_RM_LAUNCH(uint8_t, 4, true);
        else if (bits == 16) VS_RM_LAUNCH(uint16_t, 1, true);
        else VS_RM_LAUNCH(uint8_t, 1, true);
#undef VS_RM_LAUNCH
    });
    return hipGetLastError();
}

hipError_t lens_map(const vs_lens_params& p, int w, int h, int32_t* map, int map_stride, hipStream_t s) {
    if (w < 1 || h < 1 || w > 32767 || h > 32767 || !vsl::params_ok(p)) return hipErrorNotSupported;
    hipLaunchKernelGGL(vs_k_lens_map, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(256), 0, s, p, w, h, map, map_stride);
    return hipGetLastError();
}

}  // namespace vsk
