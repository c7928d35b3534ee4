// The YCbCr rule's header (video_stabilizer_amd/csrc/vs_ycbcr.hpp) against the harness programs' host conversion (apps/video_io.hpp), the rule's
// consequence (d): both directions equal on every input.  Stand-alone, host only; built with the address and undefined-behaviour sanitizers
// (tests/test_ycbcr_rule_cpp.py).  argv[1]: a directory for the small .y4m files of part 2.
//
// Part 1, the per-pixel functions: every 8-bit triple in both directions; at 10, 12 and 16 bits the extremes, the offsets +- 1 and a few
// million random triples over the whole container, BGR samples above the format's maximum among them (Writer::pack cuts those before it
// converts, and so does the rule).
// Part 2, whole frames through files: random BGR frames written by Writer::write are read back unconverted (Reader::next_planes) and held
// against vsy::frame_to_ycbcr; random planes written unconverted (Writer::write_planes) are read by Reader::next and held against
// vsy::frame_to_bgr.  4:2:0, 4:2:2, 4:4:4 and mono, 8 and 10 bit, 1 x 1, 2 x 2, 7 x 5 and 37 x 21.
// Premises, asserted at the end: some outputs clamp at 0, some at the maximum, some chroma averages round up and some round down.
#include "../../video_stabilizer_amd/csrc/vs_ycbcr.hpp"
#include "../../apps/video_io.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

long g_fail = 0, g_clamp_lo = 0, g_clamp_hi = 0, g_round_up = 0, g_round_down = 0;
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 16); }

void fail(const char* what, int bits, int a, int b, int c) {
    if (g_fail++ < 10) std::fprintf(stderr, "MISMATCH %s bits %d input %d %d %d\n", what, bits, a, b, c);
}

void check_to_bgr(int y, int cb, int cr, int bits) {
    const int sh = bits - 8, maxv = (1 << bits) - 1;
    int b0, g0, r0, b1, g1, r1;
    vsio::ycbcr_to_bgr(y, cb, cr, bits, b0, g0, r0);
    vsy::to_bgr(y, cb, cr, sh, maxv, b1, g1, r1);
    if (b0 != b1 || g0 != g1 || r0 != r1) fail("to_bgr", bits, y, cb, cr);
    const int raw = (298 * (y - (16 << sh)) + 409 * (cr - (128 << sh)) + 128) >> 8;       // the red sum before the clamp
    g_clamp_lo += raw < 0; g_clamp_hi += raw > maxv;
}
void check_to_ycbcr(int b, int g, int r, int bits) {
    const int sh = bits - 8, maxv = (1 << bits) - 1;
    int y0, u0, v0, y1, u1, v1;
    vsio::bgr_to_ycbcr(std::min(b, maxv), std::min(g, maxv), std::min(r, maxv), bits, y0, u0, v0);     // (Writer::pack's cut)
    vsy::to_ycbcr(b, g, r, sh, maxv, y1, u1, v1);
    if (y0 != y1 || u0 != u1 || v0 != v1) fail("to_ycbcr", bits, b, g, r);
}

void part1() {
    for (int a = 0; a < 256; a++)
        for (int b = 0; b < 256; b++)
            for (int c = 0; c < 256; c++) { check_to_bgr(a, b, c, 8); check_to_ycbcr(a, b, c, 8); }
    for (int bits : {10, 12, 16}) {
        const int sh = bits - 8, maxv = (1 << bits) - 1;
        std::vector<int> edge;
        for (int base : {0, 16 << sh, 128 << sh, 235 << sh, 240 << sh, maxv, 65535})
            for (int d = -1; d <= 1; d++)
                if (base + d >= 0 && base + d <= 65535) edge.push_back(base + d);
        for (int a : edge) for (int b : edge) for (int c : edge) { check_to_bgr(a, b, c, bits); check_to_ycbcr(a, b, c, bits); }
        for (long i = 0; i < 3000000; i++) {
            // the whole container, and (every other draw) the format's own range, where nothing saturates early
            const int m = (i & 1) ? 65535 : maxv;
            const int a = (int)(rnd() % (uint32_t)(m + 1)), b = (int)(rnd() % (uint32_t)(m + 1)), c = (int)(rnd() % (uint32_t)(m + 1));
            check_to_bgr(a, b, c, bits); check_to_ycbcr(a, b, c, bits);
        }
    }
}

template <typename T>
void frames(const std::string& dir, vsio::Chroma chroma, int bits, int w, int h) {
    vsio::Format fmt;
    fmt.w = w; fmt.h = h; fmt.bits = bits; fmt.chroma = chroma;
    const int sh = bits - 8, maxv = (1 << bits) - 1, top = sizeof(T) == 1 ? 255 : 65535;
    const int sub_x = chroma == vsio::Chroma::C444 || chroma == vsio::Chroma::Mono ? 0 : 1, sub_y = chroma == vsio::Chroma::C420 ? 1 : 0;
    const int cw = fmt.cw(), ch = fmt.ch();
    if (chroma != vsio::Chroma::Mono && (cw != vsy::chroma_extent(w, sub_x) || ch != vsy::chroma_extent(h, sub_y))) { fail("chroma extent", bits, w, h, 0); return; }
    const std::string path = dir + "/rule.y4m";
    // the planes of one frame in a buffer of the file's layout
    auto planes_at = [&](T* base) {
        vs_ycbcr_planes p{};
        p.y = base; p.y_stride = w; p.c_stride = cw; p.c_step = 1; p.sub_x = sub_x; p.sub_y = sub_y;
        if (chroma != vsio::Chroma::Mono) { p.cb = base + (size_t)w * h; p.cr = base + (size_t)w * h + (size_t)cw * ch; }
        return p;
    };
    // towards YCbCr: Writer::write packs, next_planes returns what it packed
    std::vector<T> bgr((size_t)w * h * 3), file(fmt.frame_samples()), mine(fmt.frame_samples(), (T)0);
    for (auto& v : bgr) v = (T)(rnd() % (uint32_t)(top + 1));
    {
        vsio::Writer wr;
        if (!wr.open(path, fmt) || !wr.write(bgr.data())) { fail("write", bits, w, h, 0); return; }
    }
    {
        vsio::Reader rd;
        if (!rd.open(path) || !rd.next_planes(file.data())) { fail("next_planes", bits, w, h, 0); return; }
    }
    vsy::frame_to_ycbcr<T>(bgr.data(), 3 * w, w, h, sh, maxv, planes_at(mine.data()));
    if (file != mine) fail("frame_to_ycbcr", bits, w, h, (int)chroma);
    // which way the averages rounded (cells of more than one pixel)
    if (sub_x + sub_y > 0)
        for (int cy = 0; cy < ch; cy++)
            for (int cx = 0; cx < cw; cx++) {
                int su = 0;
                for (int dy = 0; dy <= sub_y; dy++)
                    for (int dx = 0; dx <= sub_x; dx++) {
                        const T* s = &bgr[((size_t)std::min(cy * (1 << sub_y) + dy, h - 1) * w + std::min(cx * (1 << sub_x) + dx, w - 1)) * 3];
                        int y, cb, cr;
                        vsy::to_ycbcr(s[0], s[1], s[2], sh, maxv, y, cb, cr);
                        su += cb;
                    }
                const int cnt = 1 << (sub_x + sub_y), rem = su % cnt;
                g_round_up += rem * 2 >= cnt && rem != 0; g_round_down += rem != 0 && rem * 2 < cnt;
            }
    // towards BGR: random planes over the whole container go into the file unconverted, Reader::next unpacks them
    std::vector<T> raw(fmt.frame_samples()), got((size_t)w * h * 3), want((size_t)w * h * 3, (T)0);
    for (auto& v : raw) v = (T)(rnd() % (uint32_t)(top + 1));
    {
        vsio::Writer wr;
        if (!wr.open(path, fmt) || !wr.write_planes(raw.data())) { fail("write_planes", bits, w, h, 0); return; }
    }
    {
        vsio::Reader rd;
        if (!rd.open(path) || !rd.next(got.data())) { fail("next", bits, w, h, 0); return; }
    }
    vsy::frame_to_bgr<T>(planes_at(raw.data()), w, h, sh, maxv, want.data(), 3 * w);
    if (got != want) fail("frame_to_bgr", bits, w, h, (int)chroma);
    std::remove(path.c_str());
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: ycbcr_rule_test <scratch dir>\n"); return 2; }
    part1();
    const int sizes[4][2] = {{1, 1}, {2, 2}, {7, 5}, {37, 21}};
    long n_frames = 0;
    for (vsio::Chroma c : {vsio::Chroma::C420, vsio::Chroma::C422, vsio::Chroma::C444, vsio::Chroma::Mono})
        for (const auto& wh : sizes) {
            frames<uint8_t>(argv[1], c, 8, wh[0], wh[1]);
            frames<uint16_t>(argv[1], c, 10, wh[0], wh[1]);
            n_frames += 2;
        }
    std::printf("clamp_lo %ld clamp_hi %ld round_up %ld round_down %ld frames %ld mismatches %ld\n", g_clamp_lo, g_clamp_hi, g_round_up, g_round_down, n_frames, g_fail);
    if (g_fail) return 1;
    if (!(g_clamp_lo > 0 && g_clamp_hi > 0 && g_round_up > 0 && g_round_down > 0)) { std::fprintf(stderr, "a premise does not hold\n"); return 3; }
    std::printf("DONE\n");
    return 0;
}
