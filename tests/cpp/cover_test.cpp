// The host's "candidate 0 covers the whole window" (video_stabilizer_amd/csrc/vs_lookahead.hpp: vsi::cv_window_covered, what lets the
// stabilizer's inpaint skip a run) as a filter: every line of stdin is one case, "A B TX TY w h rx ry rw rh" -- the forward transform's four
// doubles as hex floats ("nan", "inf" as strtod reads them), then the frame and the window as ints -- and every line of stdout the decision,
// 0 or 1, taken the way Chunk::inpaint_run takes it: vs_cv_inverse_matrix, then cv_window_covered.  The cases and what the decisions are held
// against: tests/test_cover_cpp.py.  Host only: built with the address and undefined-behaviour sanitizers together with csrc/vs_host.cpp.
#include "../../video_stabilizer_amd/csrc/vs_lookahead.hpp"

#include <cstdio>
#include <cstdlib>

int main() {
    char line[1024];
    long n = 0;
    while (fgets(line, sizeof line, stdin)) {
        char* p = line;
        double d[4];
        long v[6];
        bool ok = true;
        for (int k = 0; k < 4 && ok; k++) { char* e; d[k] = strtod(p, &e); ok = e != p; p = e; }
        for (int k = 0; k < 6 && ok; k++) { char* e; v[k] = strtol(p, &e, 10); ok = e != p; p = e; }
        if (!ok) { fprintf(stderr, "line %ld: ten numbers expected\n", n + 1); return 2; }
        const vs_transform t{d[0], d[1], d[2], d[3]};
        double M[6];
        vs_cv_inverse_matrix(&t, (int)v[0], (int)v[1], M);
        printf("%d\n", vsi::cv_window_covered(M, (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[0], (int)v[1]) ? 1 : 0);
        n++;
    }
    printf("DONE %ld\n", n);
    return 0;
}
