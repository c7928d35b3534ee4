// The look-ahead passes' candidate transforms (video_stabilizer_amd/csrc/vs_lookahead.hpp) against a restatement of the rule, bit for bit.
// Host only: built with the address and undefined-behaviour sanitizers together with csrc/vs_host.cpp (tests/test_lookahead_cpp.py).
#include "../../video_stabilizer_amd/csrc/vs_lookahead.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <limits>
#include <memory>
#include <vector>

static int failures = 0;

// THE RULE: entry c is inverse(T_0 o .. o T_c), composed with the correction if there is one; the list ends at n_ahead entries, at `avail`
// queued frames or at a failed alignment, and zero transforms follow
static int expected(const std::vector<vs_transform>& meas, const std::vector<int>& ok, size_t avail, int n_ahead, const vs_transform* correction,
                    vs_transform* out) {
    vs_transform chain{0, 0, 0, 0};
    int c = 0;
    for (; c < n_ahead && (size_t)c < avail && ok[c]; c++) {
        chain = vs_transform_compose(&chain, &meas[c]);
        const vs_transform back = vs_transform_inverse(&chain);
        out[c] = correction ? vs_transform_compose(&back, correction) : back;
    }
    for (int k = c; k < n_ahead; k++) out[k] = vs_transform{0, 0, 0, 0};
    return c;
}

// one case, through the engine's containers (deques) and through heap arrays of exactly `avail` entries and n_ahead outputs: a read or a write
// behind either end is the address sanitizer's to report
static void check(const char* what, const std::vector<vs_transform>& meas, const std::vector<int>& ok, size_t avail, int n_ahead, const vs_transform* correction,
                  int want_live) {
    std::vector<vs_transform> want((size_t)n_ahead);
    const int live = expected(meas, ok, avail, n_ahead, correction, want.data());
    if (want_live >= 0 && live != want_live) { printf("FAIL %s: the restatement gives %d live, the case says %d\n", what, live, want_live); failures++; }
    const vs_transform zero{0, 0, 0, 0};
    for (int pass = 0; pass < 2; pass++) {
        std::unique_ptr<vs_transform[]> got(new vs_transform[(size_t)n_ahead]);
        memset(got.get(), 0xA5, sizeof(vs_transform) * (size_t)n_ahead);
        int n;
        if (pass == 0) {
            const std::deque<vs_transform> dm(meas.begin(), meas.end());
            const std::deque<int> dk(ok.begin(), ok.end());
            n = vsi::lookahead_transforms(dm, dk, avail, n_ahead, correction, got.get());
        } else {
            const size_t held = avail < meas.size() ? avail : meas.size();
            std::unique_ptr<vs_transform[]> am(new vs_transform[held ? held : 1]);
            std::unique_ptr<int[]> ak(new int[held ? held : 1]);
            for (size_t i = 0; i < held; i++) { am[i] = meas[i]; ak[i] = ok[i]; }
            n = vsi::lookahead_transforms(am.get(), ak.get(), held, n_ahead, correction, got.get());
        }
        bool good = n == live && memcmp(got.get(), want.data(), sizeof(vs_transform) * (size_t)n_ahead) == 0;
        for (int c = live; c < n_ahead; c++) good = good && memcmp(&got[c], &zero, sizeof zero) == 0;
        if (!good) { printf("FAIL %s (%s, n_ahead %d, avail %zu): live %d, expected %d\n", what, pass ? "arrays" : "deques", n_ahead, avail, n, live); failures++; }
    }
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const vs_transform correction{-0.013, 0.021, 7.25, -3.5};
    // twenty plausible frame-to-frame motions: small scale and rotation terms, translations of a few pixels
    std::vector<vs_transform> motion;
    for (int i = 0; i < 20; i++)
        motion.push_back(vs_transform{0.001 * (i % 5 - 2) + 1e-4 * i, 0.002 * (i % 3 - 1) - 1e-4 * i, 1.5 * (i % 7 - 3) + 0.125 * i, -2.25 * (i % 4) + 0.0625 * i});
    const std::vector<int> all_ok(20, 1);
    const vs_transform* const corrections[2] = {nullptr, &correction};
    for (const vs_transform* corr : corrections)
        for (int n_ahead : {1, 3, 16}) {
            check("nothing queued", motion, all_ok, 0, n_ahead, corr, 0);
            if (n_ahead > 1) check("fewer queued than asked for", motion, all_ok, (size_t)n_ahead - 1, n_ahead, corr, n_ahead - 1);
            check("more queued than asked for", motion, all_ok, (size_t)n_ahead + 4, n_ahead, corr, n_ahead);
            for (int bad : {0, n_ahead / 2, n_ahead - 1}) {                   // a failed alignment: first, middle, last position
                std::vector<int> ok = all_ok;
                ok[(size_t)bad] = 0;
                check("failed alignment", motion, ok, (size_t)n_ahead + 4, n_ahead, corr, bad);
                check("failed alignment at the queue's end", motion, ok, (size_t)bad + 1, n_ahead, corr, bad);
            }
            // hostile measurements: equality with the restatement and a clean sanitizer run are all that is asked
            const vs_transform hostile[] = {{nan, 0, 0, 0}, {0, 0, nan, 1}, {inf, 0, 0, 0}, {0, -inf, 2, 3}, {0, 0, inf, -inf}, {-1, 0, 5, 5} /* zero scale */,
                                            {1e308, 1e308, 1e308, 1e308}, {-1, 0, 0, 0}};
            for (const vs_transform& bad : hostile)
                for (int at : {0, n_ahead / 2, n_ahead - 1}) {
                    std::vector<vs_transform> m = motion;
                    m[(size_t)at] = bad;
                    check("hostile measurement", m, all_ok, (size_t)n_ahead + 2, n_ahead, corr, n_ahead);
                }
        }
    {   // a hostile correction
        const vs_transform bad{-1, 0, nan, inf};
        check("hostile correction", motion, all_ok, 5, 3, &bad, 3);
    }
    if (failures) { printf("%d FAILURE(S)\n", failures); return 1; }
    printf("ALL PASS\n");
    return 0;
}
