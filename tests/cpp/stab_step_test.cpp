// The stabilizer's scalar bookkeeping (video_stabilizer_amd/csrc/vs_stab_step.hpp: what vs_stabilizer.hip runs once per frame) against the oracle's
// extracted step (oracle/vs_oracle.cpp vso_stabilizer_step), bit for bit after every frame.  Host only: built with the address and
// undefined-behaviour sanitizers together with csrc/vs_host.cpp and the oracle's sources (tests/test_stab_step_cpp.py).
#include "../../video_stabilizer_amd/csrc/vs_stab_step.hpp"
#include "../../oracle/vs_oracle.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

static int failures = 0;
static const int W = 320, H = 240;

struct Frame { vs_transform meas; bool ok; bool reset_before; };

// the library's side: the fields of the handle that the step works on (vs_stabilizer.hip), reset as vs_stabilizer_reset resets them
struct Lib {
    vs_stabilizer_params p;
    vs_smoother* smoother;
    std::deque<vs_transform> measurements;
    std::deque<int> ok;
    vs_transform accum{0, 0, 0, 0};
    explicit Lib(const vs_stabilizer_params& q) : p(q), smoother(vs_smoother_create(q.lag, q.smoother_memory, q.lambda)) {}
    ~Lib() { vs_smoother_destroy(smoother); }
    void reset() {
        measurements.clear(); ok.clear();
        vs_smoother_destroy(smoother);
        smoother = vs_smoother_create(p.lag, p.smoother_memory, p.lambda);
        accum = vs_transform{0, 0, 0, 0};
    }
};

static vso_stabilizer* oracle_handle(const vs_stabilizer_params& p) {
    vso_stabilizer_params q;
    vso_stabilizer_params_default(&q);
    q.lag = p.lag; q.smoother_memory = p.smoother_memory; q.lambda = p.lambda; q.enable_smoother = p.enable_smoother;
    q.min_disp = p.min_disp; q.max_disp = p.max_disp; q.min_decay = p.min_decay; q.max_decay = p.max_decay;
    return vso_stabilizer_create(&q);
}

static vs_stabilizer_params params(int lag, int smoother) {
    vs_stabilizer_params p;
    vs_stabilizer_params_default(&p);
    p.lag = lag; p.smoother_memory = 2; p.enable_smoother = smoother;
    return p;
}

// both sides through the same frames; returns how many measurements were finalised.  accums (optional): the library's accum after every frame
static int run(const char* what, const vs_stabilizer_params& p, const std::vector<Frame>& frames, std::vector<vs_transform>* accums = nullptr) {
    static_assert(sizeof(vs_transform) == sizeof(vso_transform), "the two sides' transforms are compared as bytes");
    Lib lib(p);
    vso_stabilizer* o = oracle_handle(p);
    int finalised = 0;
    for (size_t i = 0; i < frames.size(); i++) {
        const Frame& f = frames[i];
        if (f.reset_before) { lib.reset(); vso_stabilizer_destroy(o); o = oracle_handle(p); }
        vs_transform corr;
        vso_transform ocorr, oaccum, om;
        memset(&corr, 0xA5, sizeof corr);
        memset(&ocorr, 0xA5, sizeof ocorr);
        const bool fin = vsi::stab_step(f.meas, f.ok, W, H, lib.p, lib.smoother, lib.measurements, lib.ok, lib.accum, &corr);
        memcpy(&om, &f.meas, sizeof om);
        const int ofin = vso_stabilizer_step(o, &om, f.ok ? 1 : 0, W, H, &ocorr);
        vso_stabilizer_state(o, nullptr, &oaccum, nullptr);
        bool good = (fin ? 1 : 0) == ofin && memcmp(&lib.accum, &oaccum, sizeof oaccum) == 0;
        if (fin) good = good && memcmp(&corr, &ocorr, sizeof ocorr) == 0;
        good = good && lib.ok.size() == lib.measurements.size() && lib.measurements.size() <= (size_t)p.lag;
        if (!good) {
            printf("FAIL %s, frame %zu: finalised %d / %d, accum {%a %a %a %a} / {%a %a %a %a}\n", what, i, (int)fin, ofin, lib.accum.A, lib.accum.B,
                   lib.accum.TX, lib.accum.TY, oaccum.A, oaccum.B, oaccum.TX, oaccum.TY);
            failures++;
            break;
        }
        finalised += fin ? 1 : 0;
        if (accums) accums->push_back(lib.accum);
    }
    vso_stabilizer_destroy(o);
    return finalised;
}

// plausible frame-to-frame motions, deterministic; `gain` scales the translations (large: the accumulated correction crosses the decay thresholds)
static std::vector<Frame> motions(int n, double gain, unsigned seed) {
    std::vector<Frame> f;
    unsigned x = seed;
    auto u = [&]() { x = x * 1664525u + 1013904223u; return (double)(x >> 8) / (double)(1u << 24) - 0.5; };
    for (int i = 0; i < n; i++) {
        const vs_transform t{0.004 * u(), 0.004 * u(), gain * u(), gain * u()};
        f.push_back(Frame{t, true, false});
    }
    return f;
}

static void expect(bool cond, const char* what) {
    if (!cond) { printf("FAIL %s\n", what); failures++; }
}

int main() {
    const int N = 24;
    for (int smoother : {1, 0})
        for (int lag : {1, 4, N + 6}) {                                  // (the last: longer than the sequence, nothing is ever finalised)
            const vs_stabilizer_params p = params(lag, smoother);
            char what[96];
            for (double gain : {3.0, 40.0, 400.0}) {                      // calm, around the thresholds, far beyond them
                snprintf(what, sizeof what, "smoother %d lag %d gain %g: all aligned", smoother, lag, gain);
                const int fin = run(what, p, motions(N, gain, 17));
                expect(fin == (N > lag ? N - lag : 0), "every frame past the lag finalises one measurement");
            }
            std::vector<Frame> f = motions(N, 40.0, 29);                  // failed alignments: the first two frames, a run in the middle, the last two
            for (int i : {0, 1, 9, 10, 11, N - 2, N - 1}) f[(size_t)i].ok = false;
            snprintf(what, sizeof what, "smoother %d lag %d: failed alignments", smoother, lag);
            run(what, p, f);
            f = motions(N, 40.0, 31);                                     // a reset in mid-sequence (and one on the very first frame)
            f[0].reset_before = true; f[13].reset_before = true;
            snprintf(what, sizeof what, "smoother %d lag %d: reset", smoother, lag);
            run(what, p, f);
            f = motions(N, 5.0, 37);                                      // measurements with a NaN / an infinity: equality and a clean sanitizer run
            f[5].meas.TX = std::nan(""); f[6].ok = false; f[15].meas.A = std::nan(""); f[16].meas.TY = INFINITY; f[17].ok = false;
            snprintf(what, sizeof what, "smoother %d lag %d: NaN", smoother, lag);
            run(what, p, f);
        }

    // The three decay branches on both sides of each threshold.  Smoother off, lag 1, EVERY alignment failed: accum is zero when a measurement is
    // finalised, so the new accum is the measurement itself before the decay, and for a pure translation by d along x on this 2^-30 grid the corner
    // displacement is d exactly (checked below): frame i + 1 finalises d[i].
    {
        vs_stabilizer_params p = params(1, 0);
        const double lo = p.min_disp, hi = p.max_disp, eps = std::ldexp(1.0, -30);
        const double d[] = {lo - eps, lo, lo + eps, 0.5 * (lo + hi), hi - eps, hi, hi + eps, 2 * hi, 0.0};
        const int branch[] = {0, 0, 1, 1, 1, 1, 2, 2, 0};                // 0: below or at min_disp, 1: between, 2: above max_disp
        std::vector<Frame> f;
        for (double v : d) f.push_back(Frame{vs_transform{0, 0, v, 0}, false, false});
        f.push_back(Frame{vs_transform{0, 0, 0, 0}, false, false});
        std::vector<vs_transform> accums;
        run("decay thresholds", p, f, &accums);
        for (size_t i = 0; i + 1 < f.size() && i + 1 < accums.size(); i++) {
            const double disp = vs_transform_max_corner_displacement(&f[i].meas, W, H);
            expect(disp == d[i], "the displacement of a translation on the grid is the translation");
            expect((disp > hi ? 2 : disp > lo ? 1 : 0) == branch[i], "the case lies on the side of the threshold it is meant for");
            double decay = branch[i] == 2 ? p.max_decay : p.min_decay;
            if (branch[i] == 1) {
                const double t = (disp - lo) / (hi - lo);
                decay = p.min_decay * (1.0 - t) + p.max_decay * t;
            }
            const double want = d[i] * decay;
            expect(memcmp(&accums[i + 1].TX, &want, sizeof want) == 0, "accum after a threshold case is translation x the branch's decay");
        }
    }
    if (failures) { printf("%d FAILURE(S)\n", failures); return 1; }
    printf("ALL PASS\n");
    return 0;
}
