// vs_ycbcr.hpp -- the YCbCr <-> BGR rule (include/vs_amd.h: vs_ycbcr_to_bgr_batch, vs_bgr_to_ycbcr_batch), written once for the device
// (vs_ycbcr.hip) and the host.  BT.601 limited range in 8.8 fixed point, chroma replicated towards BGR and box-averaged towards YCbCr: the
// rule of apps/video_io.hpp (vsio::ycbcr_to_bgr, vsio::bgr_to_ycbcr, Reader::unpack, Writer::pack), restated so that moving the conversion
// to the GPU changes no output file.  Integer only.  Plain C++: tests/cpp/ycbcr_rule_test.cpp builds it with g++ next to video_io.hpp.
//
// sh = bits - 8 and maxv = vs_format_max_value(format); every `>> 8` is an arithmetic shift, a floor.
//
// Hence
//
// - (a) Gray BGR (b == g == r = v) gives neutral chroma exactly: -38 - 74 + 112 == 0 and 112 - 94 - 18 == 0, so both sums are 128 >> 8 == 0.
// - (b) With no chroma planes (d == e == 0) the three to-BGR sums are the same number: b == g == r.
// - (c) Every output is defined for every input: a container holds at most 65535, so |298 c + 516 d + 128| < 2^26; BGR samples are cut
//       to maxv before they are weighted; every result is clamped to 0 .. maxv.
// - (d) Both directions equal video_io.hpp on every input (tests/cpp/ycbcr_rule_test.cpp: all 2^24 8-bit triples and whole frames).
//
// Out of scope, each a rule of its own: P010's high-bit alignment (samples sit in the LOW bits here), BT.709 and full-range matrices,
// sited chroma filters.
#pragma once

#include "../../include/vs_amd.h"

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VS_YC_HD __host__ __device__ __forceinline__
#else
#define VS_YC_HD inline
#endif

namespace vsy {

VS_YC_HD int clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one pixel to BGR; y, cb, cr: any container value
VS_YC_HD void to_bgr(int y, int cb, int cr, int sh, int maxv, int& b, int& g, int& r) {
    const int c = y - (16 << sh), d = cb - (128 << sh), e = cr - (128 << sh);
    r = clamp((298 * c + 409 * e + 128) >> 8, 0, maxv);
    g = clamp((298 * c - 100 * d - 208 * e + 128) >> 8, 0, maxv);
    b = clamp((298 * c + 516 * d + 128) >> 8, 0, maxv);
}
// one pixel to YCbCr, full resolution; b, g, r: any container value (cut to maxv first)
VS_YC_HD void to_ycbcr(int b, int g, int r, int sh, int maxv, int& y, int& cb, int& cr) {
    b = b < maxv ? b : maxv; g = g < maxv ? g : maxv; r = r < maxv ? r : maxv;
    y = clamp(((66 * r + 129 * g + 25 * b + 128) >> 8) + (16 << sh), 0, maxv);
    cb = clamp(((-38 * r - 74 * g + 112 * b + 128) >> 8) + (128 << sh), 0, maxv);
    cr = clamp(((112 * r - 94 * g - 18 * b + 128) >> 8) + (128 << sh), 0, maxv);
}
// a chroma cell's value from the sum of its (1 << sub_x) * (1 << sub_y) per-pixel values: (sum + cnt / 2) / cnt, cnt a power of two
VS_YC_HD int cell_average(int sum, int sub_x, int sub_y) {
    const int k = sub_x + sub_y;
    return (sum + ((1 << k) >> 1)) >> k;
}
VS_YC_HD int chroma_extent(int n, int sub) { return (n + sub) >> sub; }

// what both calls ask of a descriptor (the pointers apart): c_step 1 or 2, sub_* 0 or 1, rows and frames no shorter than their samples
inline bool layout_ok(const vs_ycbcr_planes& p, int n, int w, int h) {
    if ((p.c_step != 1 && p.c_step != 2) || (p.sub_x != 0 && p.sub_x != 1) || (p.sub_y != 0 && p.sub_y != 1)) return false;
    if (!p.y || !p.cb != !p.cr || p.y_stride < w) return false;
    if (n > 1 && p.y_frame_stride < (size_t)(h - 1) * (size_t)p.y_stride + (size_t)w) return false;
    if (!p.cb) return true;
    const int cw = chroma_extent(w, p.sub_x), ch = chroma_extent(h, p.sub_y);
    if (p.c_stride < cw * p.c_step) return false;
    if (n > 1 && p.c_frame_stride < (size_t)(ch - 1) * (size_t)p.c_stride + (size_t)cw * p.c_step) return false;
    return true;
}

// Whole frames on the host, pixel by pixel (T: uint8_t or uint16_t): what the kernels compute, as the tests' C++ reference reads it.
template <typename T>
inline void frame_to_bgr(const vs_ycbcr_planes& p, int w, int h, int sh, int maxv, T* dst, int dst_stride) {
    const T *Y = (const T*)p.y, *Cb = (const T*)p.cb, *Cr = (const T*)p.cr;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            int cb = 128 << sh, cr = 128 << sh;
            if (Cb) {
                const size_t ci = (size_t)(y >> p.sub_y) * p.c_stride + (size_t)(x >> p.sub_x) * p.c_step;
                cb = Cb[ci]; cr = Cr[ci];
            }
            int b, g, r;
            to_bgr(Y[(size_t)y * p.y_stride + x], cb, cr, sh, maxv, b, g, r);
            T* o = dst + (size_t)y * dst_stride + (size_t)x * 3;
            o[0] = (T)b; o[1] = (T)g; o[2] = (T)r;
        }
}
template <typename T>
inline void frame_to_ycbcr(const T* src, int src_stride, int w, int h, int sh, int maxv, const vs_ycbcr_planes& p) {
    T *Y = (T*)p.y, *Cb = (T*)p.cb, *Cr = (T*)p.cr;
    const int bx = 1 << p.sub_x, by = 1 << p.sub_y;
    for (int cy = 0; cy < chroma_extent(h, p.sub_y); cy++)
        for (int cx = 0; cx < chroma_extent(w, p.sub_x); cx++) {
            int su = 0, sv = 0;
            for (int dy = 0; dy < by; dy++)
                for (int dx = 0; dx < bx; dx++) {
                    const int x = cx * bx + dx < w - 1 ? cx * bx + dx : w - 1, y = cy * by + dy < h - 1 ? cy * by + dy : h - 1;
                    const T* s = src + (size_t)y * src_stride + (size_t)x * 3;
                    int yy, cb, cr;
                    to_ycbcr(s[0], s[1], s[2], sh, maxv, yy, cb, cr);
                    if (cx * bx + dx < w && cy * by + dy < h) Y[(size_t)y * p.y_stride + x] = (T)yy;
                    su += cb; sv += cr;
                }
            if (!Cb) continue;
            const size_t ci = (size_t)cy * p.c_stride + (size_t)cx * p.c_step;
            Cb[ci] = (T)cell_average(su, p.sub_x, p.sub_y);
            Cr[ci] = (T)cell_average(sv, p.sub_x, p.sub_y);
        }
}

}  // namespace vsy
