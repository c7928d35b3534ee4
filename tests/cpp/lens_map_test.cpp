// The host's lens map (video_stabilizer_amd/csrc/vs_host.cpp: vsi::lens_map_host, what vs_lens_map runs for VS_MEM_HOST) as a filter: every
// line of stdin is one case, thirteen doubles as hex floats ("nan", "inf" as strtod reads them) in vs_lens_params' order, then w, h and
// map_stride as ints.  The map is made in a heap block of exactly (h - 1) * map_stride + 2 w ints -- the address sanitizer's red zones lie
// right in front of pixel (0, 0) and right behind the last pixel -- whose row padding is filled with a guard value first.  Every line of stdout:
// the return code, then (code 0) the 2 w h ints of the map, then "pad" and the number of padding ints that changed.  The cases and what the
// maps are held against: tests/test_lens_map_cpp.py.  Host only: built with the address and undefined-behaviour sanitizers together with
// csrc/vs_host.cpp.
#include "../../video_stabilizer_amd/csrc/vs_internal.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main() {
    static char line[4096];
    long n = 0;
    const int32_t guard = 0x5A5A5A5A;
    while (fgets(line, sizeof line, stdin)) {
        char* p = line;
        double d[13];
        long v[3];
        bool ok = true;
        for (int k = 0; k < 13 && ok; k++) { char* e; d[k] = strtod(p, &e); ok = e != p; p = e; }
        for (int k = 0; k < 3 && ok; k++) { char* e; v[k] = strtol(p, &e, 10); ok = e != p; p = e; }
        if (!ok) { fprintf(stderr, "line %ld: sixteen numbers expected\n", n + 1); return 2; }
        const vs_lens_params lp{d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], VS_BORDER_CLAMP};
        const int w = (int)v[0], h = (int)v[1], ms = (int)v[2];
        const size_t len = w >= 1 && h >= 1 && ms >= 2 * w ? (size_t)(h - 1) * ms + 2 * (size_t)w : 1;
        int32_t* const map = new int32_t[len];
        for (size_t i = 0; i < len; i++) map[i] = guard;
        const int r = vsi::lens_map_host(&lp, w, h, map, ms);
        printf("%d", r);
        if (r == VS_OK) {
            long changed = 0;
            for (int y = 0; y < h; y++) {
                for (int x = 0; x < 2 * w; x++) printf(" %d", map[(size_t)y * ms + x]);
                for (int x = 2 * w; x < ms && y + 1 < h; x++) changed += map[(size_t)y * ms + x] != guard;
            }
            printf(" pad %ld", changed);
        }
        printf("\n");
        delete[] map;
        n++;
    }
    printf("DONE %ld\n", n);
    return 0;
}
