// The sizing of the float-tile Lanczos2 warp's per-launch tables (video_stabilizer_amd/csrc/vs_warp_table.hpp) against the rule written out
// here: one 16-byte entry per 64 x 16 output tile, then 8 bytes per output row with the rows rounded up to whole 4-row blocks.  Host only:
// built with the address and undefined-behaviour sanitizers (tests/test_warp_table_cpp.py).
#include "../../video_stabilizer_amd/csrc/vs_warp_table.hpp"

#include <cstdio>

static int failures = 0;
static void expect(bool cond, const char* what, long a = 0, long b = 0, long c = 0) {
    if (!cond) { if (failures < 40) printf("FAIL %s (%ld %ld %ld)\n", what, a, b, c); failures++; }
}

static void check(int w, int h, size_t tiles, size_t rows) {
    const vsk::WarpTableLayout L = vsk::warp_c3_table_layout(w, h);
    expect(L.tiles == tiles, "tile entries", w, h, (long)L.tiles);
    expect(L.rows == rows, "padded rows", w, h, (long)L.rows);
    expect(L.bytes == 16 * tiles + 8 * rows, "bytes", w, h, (long)L.bytes);
}

int main() {
    // the windows of tests/test_warp_tables_gpu.py, by hand
    check(64, 16, 1, 16);            // one tile
    check(65, 17, 4, 20);            // four tiles, 1-pixel remnants: 17 rows -> 20
    check(130, 37, 9, 40);           // 3 x 3 tiles, 37 rows -> 40
    check(3, 5, 1, 8);               // narrower than a column group, 5 rows -> 8
    check(61, 14, 1, 16);            // the window cut out of 130 x 37
    check(1, 1, 1, 4);
    check(1920, 1080, 30 * 68, 1080);
    check(3840, 2160, 60 * 135, 2160);
    check(0, 7, 0, 0);               // no window: nothing to reserve
    check(7, 0, 0, 0);
    check(-3, 5, 0, 0);
    // every small window against the rule: the row run covers every 4-row block that begins inside the window and nothing beyond it; the
    // frame stride keeps every frame's tables 16-byte aligned
    for (int w = 1; w <= 200; w++)
        for (int h = 1; h <= 70; h++) {
            const vsk::WarpTableLayout L = vsk::warp_c3_table_layout(w, h);
            size_t tiles = 0;
            for (int y = 0; y < h; y += 16)
                for (int x = 0; x < w; x += 64) tiles++;
            expect(L.tiles == tiles, "tiles by counting", w, h, (long)L.tiles);
            expect(L.rows % 4 == 0 && L.rows >= (size_t)h && L.rows < (size_t)h + 4, "rows: whole blocks, no more than needed", w, h, (long)L.rows);
            const size_t last_block = (size_t)(h - 1) / 4 * 4;          // first row of the last block a wave samples
            expect(last_block + 4 <= L.rows, "the last block lies inside the run", w, h, (long)L.rows);
            expect(L.bytes % 16 == 0 && L.bytes == 16 * L.tiles + 8 * L.rows, "bytes", w, h, (long)L.bytes);
        }
    // the largest frame the library takes
    const vsk::WarpTableLayout B = vsk::warp_c3_table_layout(32767, 32767);
    expect(B.tiles == (size_t)512 * 2048 && B.rows == 32768 && B.bytes == 16 * B.tiles + 8 * B.rows, "32767 x 32767");
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("ALL PASS\n");
    return 0;
}
