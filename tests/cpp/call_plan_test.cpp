// The integer rules of the kernel-level C ABI layer (video_stabilizer_amd/csrc/vs_call_plan.hpp: staging capacities, the rings' placement,
// byte spans, the window check, the index lists, frames per launch group, the alignment of the Lanczos2 tables, the runs of a fill batch),
// each against a brute-force restatement written here.  Host only: built with the address and undefined-behaviour sanitizers
// (tests/test_call_plan_cpp.py).
#define VS_CALL_PLAN_UNIT
#include "../../video_stabilizer_amd/csrc/vs_call_plan.hpp"

#include <climits>
#include <cstdio>
#include <vector>

using namespace vsi::plan;

static int failures = 0;
static void expect(bool cond, const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    if (!cond) { if (failures < 40) printf("FAIL %s (%lld %lld %lld %lld)\n", what, a, b, c, d); failures++; }
}

// ---- stage_capacity ----------------------------------------------------------------------------------
static void capacities() {
    std::vector<size_t> sizes = {0, 1, 4095, 4096, 4097, ((size_t)64 << 20) + 1, (size_t)3 << 30};
    for (int k = 12; k <= 26; k++) for (int d = -1; d <= 1; d++) sizes.push_back(((size_t)1 << k) + d);
    const size_t g = (size_t)64 << 20;
    for (size_t n : sizes) {
        const size_t c = stage_capacity(n);
        expect(c >= n, "a capacity holds its lease", (long long)n, (long long)c);
        size_t want = 4096;
        if (n <= g) { while (want < n) want *= 2; }                  // the next power of two, at least 4096
        else { want = 0; while (want < n) want += g; }               // above 64 MiB: the next multiple of 64 MiB
        expect(c == want, "the capacity is the restated one", (long long)n, (long long)c, (long long)want);
    }
}

// ---- ring placement ----------------------------------------------------------------------------------
// one take on a ring whose earlier spans are `spans`, any subset of them still busy
static void one_take(size_t head, size_t n, size_t slots, const std::vector<Span>& spans) {
    const Span sp = ring_place(head, n, slots);
    expect(sp.end - sp.begin == n && sp.end <= slots, "the span has n slots inside the ring", (long long)head, (long long)n, (long long)sp.begin);
    expect(sp.begin == (head + n > slots ? 0 : head), "the span starts at head, or at 0 exactly when it would run over the end", (long long)head, (long long)n, (long long)sp.begin);
    for (unsigned busy = 0; busy < (1u << spans.size()); busy++)
        for (size_t i = 0; i < spans.size(); i++) {
            if (!(busy >> i & 1)) continue;
            bool meets = false;                                      // the set definition: some slot lies in both
            for (size_t s = spans[i].begin; s < spans[i].end; s++) if (s >= sp.begin && s < sp.end) meets = true;
            expect(spans_overlap(sp, spans[i]) == meets, "retired first: exactly the busy spans that intersect", (long long)sp.begin, (long long)sp.end, (long long)spans[i].begin, (long long)spans[i].end);
        }
}
static void takes_from(size_t head, std::vector<Span>& spans, int depth) {
    if (depth == 5) return;
    for (size_t n = 1; n <= 8; n++) {
        one_take(head, n, 16, spans);
        const Span sp = ring_place(head, n, 16);
        spans.push_back(sp);
        takes_from(sp.end, spans, depth + 1);
        spans.pop_back();
    }
}
static void ring_rules() {
    std::vector<Span> spans;
    takes_from(0, spans, 0);
    for (size_t slots : {kParamSlots, kTableInts}) {
        const size_t n = slots / 2;
        expect(take_fits(n, slots) && take_fits(1, slots) && !take_fits(n + 1, slots) && !take_fits(0, slots), "a take is 1 .. half the ring", (long long)slots);
        for (size_t head : {slots - n, slots - n + 1, (size_t)0}) one_take(head, n, slots, {});
        expect(ring_place(slots - n, n, slots).begin == slots - n && ring_place(slots - n + 1, n, slots).begin == 0, "the last fit and the first wrap", (long long)slots);
    }
    expect(kParamSlots == 32768 && kTableInts == (size_t)8 << 20, "the rings' sizes");
}

// ---- spans -------------------------------------------------------------------------------------------
static void spans() {
    for (int w : {1, 2, 65535})
        for (int h : {1, 2, 3})
            for (int ch : {1, 3})
                for (int bits : {8, 10, 16})
                    for (int pad : {0, 1, 5})
                        for (int n : {1, 3})
                            for (int gap : {0, 7}) {
                                const int stride = w * ch + pad;
                                const size_t esz = bits == 8 ? 1 : 2;
                                const size_t fs = img_span(w, h, stride, ch) + gap;
                                size_t last = 0;                     // the highest byte index a pixel-by-pixel walk touches
                                for (int f = 0; f < n; f++)
                                    for (int y = 0; y < h; y++)
                                        for (int x = 0; x < w; x++)
                                            for (int c = 0; c < ch; c++)
                                                last = std::max(last, ((size_t)f * fs + (size_t)y * stride + (size_t)x * ch + c) * esz + esz - 1);
                                const Batch b{nullptr, fs, n, w, h, stride, ch, bits};
                                expect(b.esz() == esz && b.bytes() == last + 1, "the byte span of a batch", w, h, n, (long long)b.bytes());
                                expect(b.strides_ok(), "rows and frames that do not overlap are accepted", w, h, n);
                                expect(!Batch{nullptr, fs, n, w, h, w * ch - 1, ch, bits}.strides_ok(), "a row stride below the row is refused", w, ch);
                                expect(Batch{nullptr, fs - gap - 1, n, w, h, stride, ch, bits}.strides_ok() == (n == 1), "a frame stride below the span is refused", w, h, n);
                            }
}
static void out_images() {
    for (size_t row = 1; row <= 4; row++)
        for (size_t rows = 1; rows <= 3; rows++)
            for (size_t pitch = row; pitch <= row + 2; pitch++)
                for (size_t frames = 1; frames <= 3; frames++)
                    for (size_t extra = 0; extra <= 4; extra++) {
                        const size_t fp = (rows - 1) * pitch + row + extra;      // from the frame's span on: rows * pitch is among them
                        std::vector<char> hit((frames - 1) * fp + rows * pitch + 1, 0);
                        size_t last = 0;
                        for (size_t f = 0; f < frames; f++)
                            for (size_t r = 0; r < rows; r++)
                                for (size_t k = 0; k < row; k++) { hit[f * fp + r * pitch + k] = 1; last = f * fp + r * pitch + k; }
                        bool gap = false;
                        for (size_t k = 0; k <= last; k++) if (!hit[k]) gap = true;
                        const bool dense = out_image_dense(row, rows, pitch, frames, fp);
                        expect(out_image_bytes(row, rows, pitch, frames, fp) == last + 1, "an image output's byte count", (long long)row, (long long)rows, (long long)pitch, (long long)frames);
                        expect(!dense || !gap, "dense only when the walk leaves no gap", (long long)row, (long long)rows, (long long)pitch, (long long)fp);
                        // a single row per frame has no pitch to speak of, and the rule still asks pitch == row_bytes of it: exact from two rows on
                        if (rows >= 2 || pitch == row) expect(dense == !gap, "dense exactly when the walk leaves no gap", (long long)row, (long long)rows, (long long)pitch, (long long)fp);
                    }
    expect(out_image_bytes(4, 0, 4, 2, 8) == 0 && out_image_bytes(4, 2, 4, 0, 8) == 0, "no rows or no frames: no bytes");
}

// ---- window check ------------------------------------------------------------------------------------
static void windows() {
    std::vector<int> v;
    for (int k = -1; k <= 9; k++) v.push_back(k);
    v.push_back(INT_MAX); v.push_back(INT_MAX - 1);
    const int W = 8, H = 8;
    for (int x : v) for (int y : v) for (int rw : v) for (int rh : v) {
        const long long X = x, Y = y, RW = rw, RH = rh;
        const bool wide = RW >= 1 && RH >= 1 && X >= 0 && Y >= 0 && X + RW <= W && Y + RH <= H;   // (64-bit: no sum overflows)
        expect(window_ok(x, y, rw, rh, W, H) == wide, "the window check", x, y, rw, rh);
        if (x <= 9 && y <= 9 && rw <= 9 && rh <= 9) {                // the set definition: at least a pixel, every pixel in the frame
            bool inside = rw >= 1 && rh >= 1;
            for (int j = 0; j < rh; j++) for (int i = 0; i < rw; i++) if (x + i < 0 || x + i >= W || y + j < 0 || y + j >= H) inside = false;
            expect(wide == inside, "the restatement is the set definition", x, y, rw, rh);
        }
    }
}

// ---- CandIndex ---------------------------------------------------------------------------------------
static bool check_restated(const std::vector<int32_t>& l, int n_out, int n_cand, int n_src, bool behind_end) {
    for (int o = 0; o < n_out; o++) {
        bool ended = false;
        for (int c = 0; c < n_cand; c++) {
            const int32_t k = l[(size_t)o * n_cand + c];
            if (c == 0 && k < 0) return false;
            if (k < 0) ended = true;
            if ((!ended || behind_end) && k >= n_src) return false;
        }
    }
    return true;
}
static void cand_index() {
    const int n_out = 2, n_src = 5;
    const size_t stride = 24;
    const char* const base = (const char*)0x10000;
    for (int n_cand : {1, 2, 16})
        for (int cut = 0; cut <= n_cand; cut++)                      // (cut == n_cand: the list is full)
            for (int bad = -1; bad < n_cand; bad++) {                // (an index == n_src at `bad`; -1: nowhere)
                std::vector<int32_t> l((size_t)n_out * n_cand);
                for (int o = 0; o < n_out; o++)
                    for (int c = 0; c < n_cand; c++) l[(size_t)o * n_cand + c] = c == cut ? -1 : (o + 2 * c) % n_src;
                if (bad >= 0 && bad != cut) l[(size_t)n_cand + bad] = n_src;    // (in the second list)
                const CandIndex idx{l.data(), n_out, n_cand};
                for (bool behind : {false, true})
                    expect(idx.check(n_src, behind) == check_restated(l, n_out, n_cand, n_src, behind), "check is the restated rule", n_cand, cut, bad, behind);
                if (cut == 0) expect(!idx.check(n_src, false) && !idx.check(n_src, true), "candidate 0 negative is rejected", n_cand);
                if (cut > 0 && bad > cut) expect(!idx.check(n_src, true) && idx.check(n_src, false), "n_src behind the cut: rejected with behind_end only", n_cand, cut, bad);
                if (cut > 0 && bad >= 0 && bad < cut) expect(!idx.check(n_src, true) && !idx.check(n_src, false), "n_src before the cut is rejected", n_cand, cut, bad);
                if (cut == 0 || (bad >= 0 && bad < cut)) continue;   // (pointers is for checked lists)
                const std::vector<const char*> p = idx.pointers<char>(base, stride);
                expect(p.size() == l.size(), "a pointer per entry");
                for (int o = 0; o < n_out; o++)
                    for (int c = 0; c < n_cand; c++) {
                        const size_t i = (size_t)o * n_cand + c;
                        expect(p[i] == (c >= cut ? nullptr : base + (size_t)l[i] * stride), "null from the cut on, else base + k * stride", n_cand, cut, o, c);
                    }
            }
}

// ---- frames per group --------------------------------------------------------------------------------
static void group_sizes() {
    const size_t half = kParamSlots / 2, thalf = kTableInts / 2;
    for (int n_cand = 1; n_cand <= 16; n_cand++)
        for (int width : {4, 5}) {
            const int per = frames_per_group_entries(n_cand, width);
            const size_t entries = (size_t)per * n_cand, ratios = width == 5 ? (entries + 3) / 4 : 0;     // (a float per entry, in float4 slots)
            expect(per >= 1, "a group has a frame", n_cand, width);
            expect(entries * 4 + ratios <= half && take_fits(entries * 4, kParamSlots), "a group's entries and ratios fit half the ring", n_cand, width, per);
            expect(((size_t)per + 1) * n_cand * width > half, "one frame more does not fit at the rule's width", n_cand, width, per);
        }
    const int mper = frames_per_group_matrices();
    expect(matrix_slots(mper) <= half && matrix_slots((size_t)mper + 1) > half, "the matrices of a group fit half the ring, one frame more does not", mper);
    expect(matrix_slots(1) == 3 && matrix_slots(2) == 6 && matrix_slots(3) == 9, "three slots per frame");
    for (int fill = 0; fill <= 16; fill++)
        for (size_t tab : {(size_t)0, (size_t)1, thalf, thalf + 1}) {
            size_t want = half / 3;                                                  // section 19's table: the minimum of the three rules
            if (fill) want = std::min(want, half / 4 / fill);
            if (tab) want = std::min(want, std::max<size_t>(1, thalf / tab));
            const int per = frames_per_group_cv(fill, tab);
            expect(per >= 1 && (size_t)per == want, "the fixed-point route's limit is the minimum of the three rules", fill, (long long)tab, per);
            if (tab && tab <= thalf) expect((size_t)per * tab <= thalf, "the group's tables fit half the table ring", fill, (long long)tab, per);
        }
    expect(frames_per_group_tables(100, thalf) == 1 && frames_per_group_tables(100, thalf + 1) == 1 && frames_per_group_tables(100, 1) == 100
           && frames_per_group_tables(100, 0) == 100 && frames_per_group_tables(100, thalf / 2) == 2, "the table limit at its edges");
}

// ---- the Lanczos2 tables' alignment ------------------------------------------------------------------
static void table_alignment() {
    const size_t thalf = kTableInts / 2;
    for (size_t ints : {(size_t)1, (size_t)5, (size_t)1000, thalf - 3})
        for (uintptr_t base = 0x7000; base < 0x7040; base += 4) {    // a span starts on any dword
            const uintptr_t a = align16(base);
            expect(a % 16 == 0 && a >= base && a - base < 16, "the next 16-byte boundary", (long long)base, (long long)a);
            expect(a + ints * 4 <= base + aligned_table_take(ints) * 4, "the aligned tables lie inside the span taken", (long long)base, (long long)ints);
        }
    expect(!aligned_tables_fit(0) && aligned_tables_fit(1) && aligned_tables_fit(thalf - 3) && !aligned_tables_fit(thalf - 2), "tables with their spare ints against half the ring");
}

// ---- run partition -----------------------------------------------------------------------------------
static void runs() {
    const int n_out = 6;
    for (int n_cand : {1, 3})
        for (unsigned pat = 0; pat < 32; pat++) {                    // bit e - 1: output e's own frame follows output e - 1's
            std::vector<int32_t> l((size_t)n_out * n_cand, 7);
            l[0] = 10;
            for (int e = 1; e < n_out; e++) l[(size_t)e * n_cand] = l[(size_t)(e - 1) * n_cand] + ((pat >> (e - 1) & 1) ? 1 : (e % 2 ? 3 : -2));
            const CandIndex idx{l.data(), n_out, n_cand};
            int j = 0, steps = 0;
            while (j < n_out && steps++ < 10) {
                const int e = idx.run_end(j);
                expect(e > j && e <= n_out, "a run has an output and ends inside the batch", pat, j, e);
                for (int k = j + 1; k < e; k++) expect(pat >> (k - 1) & 1, "inside a run every frame follows the previous one", pat, j, e, k);
                if (e < n_out) expect(!(pat >> (e - 1) & 1), "a run is maximal", pat, j, e);
                j = e;
            }
            expect(j == n_out, "the runs tile the batch", pat, j);
        }
}

int main() {
    capacities();
    ring_rules();
    spans();
    out_images();
    windows();
    cand_index();
    group_sizes();
    table_alignment();
    runs();
    printf(failures ? "%d FAILURES\n" : "ALL PASS\n", failures);
    return failures ? 1 : 0;
}
