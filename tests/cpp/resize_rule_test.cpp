// THE RESIZE RULE's header (video_stabilizer_amd/csrc/vs_resize.hpp) on its own.  Stand-alone, host only; built with the address and
// undefined-behaviour sanitizers (tests/test_resize_rule_cpp.py), so a 64-bit product that overflowed at 32767 would end the run.
//
// Every (s, d) with both up to 512, and the large sizes 1920, 3712, 3840 and 32767 against a handful of destinations, under both filters:
//   - validity: LINEAR takes every pair in range; AREA exactly d <= s <= 8 d (both sides of s == 8 d and of d == s are among the pairs);
//   - every table entry: n >= 1, weights sum to 4096, 0 <= i0 and i0 + n <= s, LINEAR n <= 2 with no zero weight, AREA n <= floor(s / d) + 2
//     and n <= 9; i0 and i0 + n never decrease along the axis (the tiled kernel takes a tile's source rows from its first and last entry);
//     d == s is the identity table;
//   - the launch shape: for R = resize_tile_rows(s, d, filter) every tile of R destination rows touches at most source_rows_bound rows, and
//     that many rows fit kLdsBytes; R is 16 wherever 16 rows fit.
// Known answers: LINEAR 4 -> 8 and AREA 7 -> 3 as the rule's text has them.
#include "../../video_stabilizer_amd/csrc/vs_resize.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

long g_fail = 0, g_pairs = 0, g_entries = 0, g_small_tiles = 0, g_two_tap = 0, g_nine_tap = 0;

void fail(const char* what, int s, int dn, int filter, int d) {
    if (g_fail++ < 10) std::fprintf(stderr, "FAIL %s: s %d d %d filter %d entry %d\n", what, s, dn, filter, d);
}

void check_pair(int s, int dn, int filter) {
    const bool want = filter == vsr::kLinear || (dn <= s && s <= 8 * (long long)dn);
    if (vsr::resize_axis_valid(s, dn, filter) != want) fail("validity", s, dn, filter, -1);
    if (!want) return;
    g_pairs++;
    std::vector<int> first(dn), count(dn);
    for (int d = 0; d < dn; d++) {
        uint16_t wt[vsr::kMaxTaps + 2];
        for (auto& w : wt) w = 0xffff;
        int i0 = -1;
        const int n = vsr::resize_taps(s, dn, filter, d, &i0, wt);
        g_entries++;
        if (n < 1 || n > vsr::kMaxTaps - 1) { fail("count", s, dn, filter, d); return; }
        long sum = 0;
        for (int k = 0; k < n; k++) sum += wt[k];
        if (sum != vsr::kOne) fail("sum", s, dn, filter, d);
        if (wt[n] != 0xffff) fail("write past the count", s, dn, filter, d);
        if (i0 < 0 || i0 + n > s) fail("range", s, dn, filter, d);
        if (filter == vsr::kLinear) {
            if (n > 2 || wt[0] == 0 || (n == 2 && wt[1] == 0)) fail("linear taps", s, dn, filter, d);
            g_two_tap += n == 2;
        } else {
            if (n > s / dn + 2) fail("area taps", s, dn, filter, d);
            g_nine_tap += n == 9;
        }
        if (s == dn && (i0 != d || n != 1)) fail("identity", s, dn, filter, d);
        if (d > 0 && (i0 < first[d - 1] || i0 + n < first[d - 1] + count[d - 1])) fail("monotone", s, dn, filter, d);
        first[d] = i0; count[d] = n;
    }
    // the launch shape
    const int R = vsr::resize_tile_rows(s, dn, filter);
    const long long bound = vsr::source_rows_bound(s, dn, filter, R);
    if (R < 1 || R > vsr::kMaxTileRows || (R & (R - 1))) fail("tile rows", s, dn, filter, R);
    if (bound * vsr::kLdsRowBytes > vsr::kLdsBytes) fail("LDS bytes", s, dn, filter, R);
    if (R < vsr::kMaxTileRows && vsr::source_rows_bound(s, dn, filter, 2 * R) <= vsr::kLdsRows) fail("tile rows not the largest", s, dn, filter, R);
    g_small_tiles += R < vsr::kMaxTileRows;
    for (int e0 = 0; e0 < dn; e0 += R) {
        const int e1 = e0 + R < dn ? e0 + R : dn;
        const int rows = first[e1 - 1] + count[e1 - 1] - first[e0];
        if (rows < 1 || rows > bound) fail("source rows of a tile", s, dn, filter, e0);
    }
}

void known_answers() {
    const int lin[8][3] = {{0, 4096, 0}, {0, 3072, 1024}, {0, 1024, 3072}, {1, 3072, 1024}, {1, 1024, 3072}, {2, 3072, 1024}, {2, 1024, 3072}, {3, 4096, 0}};
    for (int d = 0; d < 8; d++) {
        uint16_t wt[vsr::kMaxTaps] = {0};
        int i0 = -1;
        const int n = vsr::resize_taps_linear(4, 8, d, &i0, wt);
        if (i0 != lin[d][0] || wt[0] != lin[d][1] || n != (lin[d][2] ? 2 : 1) || (n == 2 && wt[1] != lin[d][2])) fail("LINEAR 4 -> 8", 4, 8, 0, d);
    }
    const int area[3][4] = {{0, 1755, 1756, 585}, {2, 1170, 1756, 1170}, {4, 585, 1756, 1755}};
    for (int d = 0; d < 3; d++) {
        uint16_t wt[vsr::kMaxTaps] = {0};
        int i0 = -1;
        const int n = vsr::resize_taps_area(7, 3, d, &i0, wt);
        if (n != 3 || i0 != area[d][0] || wt[0] != area[d][1] || wt[1] != area[d][2] || wt[2] != area[d][3]) fail("AREA 7 -> 3", 7, 3, 1, d);
    }
}

}  // namespace

int main() {
    known_answers();
    for (int filter = 0; filter < 2; filter++) {
        for (int s = 1; s <= 512; s++)
            for (int dn = 1; dn <= 512; dn++) check_pair(s, dn, filter);
        const int large[] = {1920, 3712, 3840, 32767};
        for (int s : large) {
            const int dst[] = {1, 1080, 1920, 2160, 3840, s - 1, s, s + 1, (s + 7) / 8, (s + 7) / 8 - 1, s / 2, 32767};
            for (int dn : dst)
                if (dn >= 1 && dn <= vsr::kMaxExtent) check_pair(s, dn, filter);
        }
        check_pair(1, 32767, filter);
        check_pair(4096, 32767, filter);
    }
    // the ends of the validity range, and the filters that do not exist
    if (vsr::resize_axis_valid(0, 4, 0) || vsr::resize_axis_valid(4, 0, 0) || vsr::resize_axis_valid(32768, 4, 0) || vsr::resize_axis_valid(4, 32768, 0) ||
        vsr::resize_axis_valid(4, 4, 2) || vsr::resize_axis_valid(4, 4, -1) || !vsr::resize_params_valid(8, 64, 1, 8, 1) || vsr::resize_params_valid(9, 64, 1, 8, 1) ||
        vsr::resize_params_valid(8, 65, 1, 8, 1) || !vsr::resize_params_valid(9, 65, 1, 8, 0))
        fail("validity ends", 0, 0, 0, 0);
    // premises: the sweep met two-tap LINEAR entries, nine-tap AREA entries and shapes whose tile is lower than 16 rows
    if (!g_two_tap || !g_nine_tap || !g_small_tiles) fail("premises", (int)g_two_tap, (int)g_nine_tap, (int)g_small_tiles, 0);
    std::printf("pairs %ld entries %ld small-tile shapes %ld failures %ld\n", g_pairs, g_entries, g_small_tiles, g_fail);
    std::printf("DONE\n");
    return g_fail ? 1 : 0;
}
