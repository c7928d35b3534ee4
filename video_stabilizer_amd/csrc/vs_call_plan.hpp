// vs_call_plan.hpp -- the parts of the kernel-level C ABI layer (vs_runtime.hip, vs_capi.hip, vs_capi_warp.hip, vs_capi_lookahead.hip) that are
// pure functions of integers: staging capacities, where the span rings place a take, byte spans of images and batches, the window check, the
// index lists of the look-ahead entry points, how many frames go into one launch group, and the runs of a fill batch.  Each rule is written
// once, here.  Host only, no HIP, no locks, no events: tests/cpp/call_plan_test.cpp builds it with plain g++.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#ifndef VS_CALL_PLAN_UNIT
#error "vs_call_plan.hpp belongs to the C ABI layer (vs_capi.hpp) and tests/cpp/call_plan_test.cpp only (they define VS_CALL_PLAN_UNIT)"
#endif
namespace vsi {
namespace plan {

// ---- staging pool: the capacity of the block that serves a lease of n bytes ------------------------------------------------------
// rounded up so that a sweep of slightly different sizes reuses blocks: powers of two from 4 KiB to 64 MiB, multiples of 64 MiB above
inline size_t stage_capacity(size_t n) {
    if (n <= 4096) return 4096;
    if (n <= ((size_t)64 << 20)) { size_t c = 4096; while (c < n) c <<= 1; return c; }
    const size_t g = (size_t)64 << 20;
    return (n + g - 1) / g * g;
}

// ---- span rings ------------------------------------------------------------------------------------------------------------------
constexpr size_t kParamSlots = (size_t)1 << 15;   // the parameter ring: 32768 float4 = 512 KiB
constexpr size_t kTableInts = (size_t)8 << 20;    // the table ring: 32 MiB, ~680 4K frames of VS_WARP_BILINEAR_CV coordinate tables
struct Span { size_t begin, end; };
// the largest take a ring of `slots` units serves: half the ring, so that a call never waits for its own previous span
inline bool take_fits(size_t n, size_t slots) { return n != 0 && n <= slots / 2; }
// where a take of n units goes in a ring whose last span ended at `head`: behind it, or at 0 when it would run over the end
inline Span ring_place(size_t head, size_t n, size_t slots) {
    const size_t b = head + n > slots ? 0 : head;
    return Span{b, b + n};
}
// a span that is still in flight has to be retired before `s` is handed out
inline bool spans_overlap(const Span& s, const Span& busy) { return busy.begin < s.end && s.begin < busy.end; }

// ---- byte spans ------------------------------------------------------------------------------------------------------------------
// elements from the first pixel of a w x h image with rows of `stride` elements to behind its last
inline size_t img_span(int w, int h, int stride, int channels) { return (size_t)(h - 1) * stride + (size_t)w * channels; }
inline size_t elem_size(int bits) { return bits > 8 ? 2 : 1; }
// a batch of images somewhere: n images of w x h pixels of `channels` elements of `bits` bits, rows of `stride` elements, `fs` elements from
// image to image (not looked at for n == 1)
struct Batch {
    const void* p;
    size_t fs;
    int n, w, h, stride, channels, bits;
    size_t esz() const { return elem_size(bits); }
    size_t bytes() const { return ((size_t)(n - 1) * fs + img_span(w, h, stride, channels)) * esz(); }
    // rows hold their pixels and images do not overlap
    bool strides_ok() const { return stride >= w * channels && (n == 1 || fs >= img_span(w, h, stride, channels)); }
};
// an image output of `frames` images of `rows` rows of `row_bytes` bytes, `pitch` bytes from row to row, `frame_pitch` from image to image
inline size_t out_image_bytes(size_t row_bytes, size_t rows, size_t pitch, size_t frames, size_t frame_pitch) {
    return frames == 0 || rows == 0 ? 0 : (frames - 1) * frame_pitch + (rows - 1) * pitch + row_bytes;
}
// no gap between rows or between images: the output travels back as it lies
inline bool out_image_dense(size_t row_bytes, size_t rows, size_t pitch, size_t frames, size_t frame_pitch) {
    return pitch == row_bytes && (frames <= 1 || frame_pitch == rows * pitch);
}

// ---- the output window -----------------------------------------------------------------------------------------------------------
// a window of at least a pixel inside the w x h frame (no sum that could overflow)
inline bool window_ok(int x, int y, int rw, int rh, int w, int h) {
    return x >= 0 && y >= 0 && rw >= 1 && rh >= 1 && rw <= w && rh <= h && x <= w - rw && y <= h - rh;
}

// ---- the index-based entry points' lists -----------------------------------------------------------------------------------------
// cand_frame[o * n_cand + c] is a frame of the batch at `src`, a negative index ends a list
struct CandIndex {
    const int32_t* cand_frame;
    int n_out, n_cand;
    // candidate 0 is the frame itself and no index reaches n_src; behind_end: neither does one behind a negative index (the fill's and the deblur's
    // rule; the denoise and the exposure statistics do not read there)
    bool check(int n_src, bool behind_end) const {
        for (int o = 0; o < n_out; o++) {
            const int32_t* row = cand_frame + (size_t)o * n_cand;
            if (row[0] < 0) return false;
            for (int c = 0; c < n_cand && (behind_end || row[c] >= 0); c++) if (row[c] >= n_src) return false;
        }
        return true;
    }
    // index k -> base + k * stride bytes (a frame; a frame's sharpness; its three sums), null from the end of a list on
    template <typename T> std::vector<const T*> pointers(const void* base, size_t stride) const {
        std::vector<const T*> p((size_t)n_out * n_cand, nullptr);
        for (int i = 0; i < n_out; i++)
            for (int c = 0; c < n_cand && cand_frame[(size_t)i * n_cand + c] >= 0; c++)
                p[(size_t)i * n_cand + c] = (const T*)((const char*)base + (size_t)cand_frame[(size_t)i * n_cand + c] * stride);
        return p;
    }
    // the run of outputs from j on whose own frames are consecutive in the batch: [j, end)
    int run_end(int j) const {
        int e = j + 1;
        while (e < n_out && cand_frame[(size_t)e * n_cand] == cand_frame[(size_t)(e - 1) * n_cand] + 1) e++;
        return e;
    }
};

// ---- frames per launch group ("frames per group") ----------------------------------------------------------
// what a group sends has to fit one take: half the ring
// the inverted matrices of VS_WARP_BILINEAR_CV: six doubles = three slots per frame, an upload counted in 16-byte slots
inline size_t matrix_slots(size_t frames) { return (frames * 6 * sizeof(double) + 15) / 16; }
inline int frames_per_group_matrices() { return (int)(kParamSlots / 2 / 3); }
// candidate entries: n_cand per frame, four slots each; five where the pass takes a ratio per entry next to them (the deblur)
inline int frames_per_group_entries(int n_cand, int slots_per_entry) { return std::max(1, (int)(kParamSlots / 2 / (size_t)slots_per_entry) / n_cand); }
// coordinate tables of table_ints per frame (0: the route has none) against half the table ring; a frame whose tables do not fit goes alone and
// takes the route without tables
inline int frames_per_group_tables(int limit, size_t table_ints) {
    return table_ints ? (int)std::min<size_t>((size_t)limit, std::max<size_t>(1, kTableInts / 2 / table_ints)) : limit;
}
// the fixed-point route: matrices, (fill_cand != 0: with the fill's pass 2) entries, tables
inline int frames_per_group_cv(int fill_cand, size_t table_ints) {
    int per = frames_per_group_matrices();
    if (fill_cand) per = std::min(per, frames_per_group_entries(fill_cand, 4));
    return frames_per_group_tables(per, table_ints);
}

// ---- the Lanczos2 route's per-launch tables --------------------------------------------------------------------------------------
// taken from the table ring with three ints to spare, so that a 16-byte aligned start lies inside the span whatever dword the span starts on
inline size_t aligned_table_take(size_t table_ints) { return table_ints + 3; }
inline bool aligned_tables_fit(size_t table_ints) { return table_ints && aligned_table_take(table_ints) <= kTableInts / 2; }
inline uintptr_t align16(uintptr_t p) { return (p + 15) & ~(uintptr_t)15; }

}  // namespace plan
}  // namespace vsi
