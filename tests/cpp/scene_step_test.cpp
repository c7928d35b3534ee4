// The stabilizer's step with scene cuts (video_stabilizer_amd/csrc/vs_stab_step.hpp: stab_step_cut, what vs_stabilizer.hip runs once per frame)
// against stab_step, bit for bit, where no frame is a cut, and on hand-worked sequences with a cut.  Host only: built with the address and
// undefined-behaviour sanitizers together with csrc/vs_host.cpp (tests/test_scene_step_cpp.py).
#include "../../video_stabilizer_amd/csrc/vs_stab_step.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

static int failures = 0;
static const int W = 320, H = 240;

static void expect(bool cond, const char* what, int a = -1, int b = -1) {
    if (!cond) { printf("FAIL %s (%d, %d)\n", what, a, b); failures++; }
}
static bool same(const vs_transform& a, const vs_transform& b) { return memcmp(&a, &b, sizeof a) == 0; }

// the fields of the handle that the step works on (vs_stabilizer.hip)
struct Side {
    vs_stabilizer_params p;
    vs_smoother* smoother;
    std::deque<vs_transform> measurements;
    std::deque<int> ok, cuts;
    vs_transform accum{0, 0, 0, 0};
    explicit Side(const vs_stabilizer_params& q) : p(q), smoother(vs_smoother_create(q.lag, q.smoother_memory, q.lambda)) {}
    ~Side() { vs_smoother_destroy(smoother); }
};

static vs_stabilizer_params params(int lag, int smoother) {
    vs_stabilizer_params p;
    vs_stabilizer_params_default(&p);
    p.lag = lag; p.smoother_memory = 2; p.enable_smoother = smoother;
    return p;
}

struct Frame { vs_transform meas; bool ok; bool cut; };

// plausible frame-to-frame motions, deterministic; `gain` scales the translations
static std::vector<Frame> motions(int n, double gain, unsigned seed) {
    std::vector<Frame> f;
    unsigned x = seed;
    auto u = [&]() { x = x * 1664525u + 1013904223u; return (double)(x >> 8) / (double)(1u << 24) - 0.5; };
    for (int i = 0; i < n; i++) f.push_back(Frame{vs_transform{0.004 * u(), 0.004 * u(), gain * u(), gain * u()}, true, false});
    return f;
}

// no cut anywhere: stab_step_cut is stab_step, bit for bit, after every frame
static void no_cut_is_stab_step(const char* what, const vs_stabilizer_params& p, const std::vector<Frame>& frames) {
    Side a(p), b(p);
    for (size_t i = 0; i < frames.size(); i++) {
        vs_transform ca, cb;
        memset(&ca, 0xA5, sizeof ca);
        memset(&cb, 0xA5, sizeof cb);
        const bool fa = vsi::stab_step(frames[i].meas, frames[i].ok, W, H, a.p, a.smoother, a.measurements, a.ok, a.accum, &ca);
        const bool fb = vsi::stab_step_cut(frames[i].meas, frames[i].ok, false, W, H, b.p, b.smoother, b.measurements, b.ok, b.cuts, b.accum, &cb);
        bool good = fa == fb && same(a.accum, b.accum) && same(ca, cb) && a.ok == b.ok && a.measurements.size() == b.measurements.size() &&
                    b.cuts.size() == b.measurements.size();
        for (size_t k = 0; good && k < a.measurements.size(); k++) good = same(a.measurements[k], b.measurements[k]) && b.cuts[k] == 0;
        if (!good) { printf("FAIL %s, frame %zu\n", what, i); failures++; return; }
    }
}

// A sequence with one cut at frame `at`, lag `lag`: what the rule says about accum, ok and the corrections, and -- the frames behind the cut --
// equality with a fresh handle that starts at the cut frame with the identity as its first measurement.
static void one_cut(int lag, int smoother, int at, bool cut_also_failed) {
    const int N = 20;
    const vs_stabilizer_params p = params(lag, smoother);
    std::vector<Frame> f = motions(N, 40.0, 41 + (unsigned)lag);
    f[(size_t)at].cut = true;
    f[(size_t)at].ok = !cut_also_failed;
    Side s(p), plain(p);
    const vs_transform ident{0, 0, 0, 0};
    const vs_transform inv_ident = vs_transform_inverse(&ident);
    for (int i = 0; i < N; i++) {
        const vs_transform before = s.accum;
        vs_transform corr, pc;
        memset(&corr, 0xA5, sizeof corr);
        const bool fin = vsi::stab_step_cut(f[(size_t)i].meas, f[(size_t)i].ok, f[(size_t)i].cut, W, H, s.p, s.smoother, s.measurements, s.ok, s.cuts, s.accum, &corr);
        expect(fin == (i >= lag), "every frame past the lag finalises one measurement", lag, i);
        expect(s.ok.size() == s.measurements.size() && s.cuts.size() == s.measurements.size() && (int)s.measurements.size() <= lag, "the three queues run together", lag, i);
        // the old scene's frames, finalised before the cut frame arrives, come out as without detection
        if (i < at) {
            const bool pf = vsi::stab_step(f[(size_t)i].meas, f[(size_t)i].ok, W, H, plain.p, plain.smoother, plain.measurements, plain.ok, plain.accum, &pc);
            expect(pf == fin && same(plain.accum, s.accum) && (!fin || same(pc, corr)), "in front of the cut nothing differs", lag, i);
        }
        if (i == at) {
            // on arrival: the identity enters the queue with ok == 0; accum is left alone unless the alignment failed too or (lag 0) the cut frame is
            // finalised at once
            if (lag > 0) {
                expect(same(s.measurements.back(), ident) && s.ok.back() == 0 && s.cuts.back() == 1, "the cut frame is queued as the identity with ok 0", lag, i);
                if (cut_also_failed) expect(!fin ? same(s.accum, ident) : true, "a failed cut frame resets accum on arrival as well", lag, i);
                else if (!fin) expect(same(s.accum, before), "accum is untouched on arrival (nothing finalised)", lag, i);
            }
        }
        // the frames of the old scene that are finalised while the cut frame waits: accum moves as the step moves it, never to the identity by the cut
        if (i > at && i < at + lag && !cut_also_failed && fin) expect(!same(s.accum, ident), "accum is not reset while the cut frame waits", lag, i);
        if (i == at + lag) {                                              // the cut frame itself is finalised
            expect(fin && same(s.accum, ident), "accum is the identity when the cut frame is finalised", lag, i);
            expect(same(corr, inv_ident), "the cut frame's correction is inverse(identity)", lag, i);
            expect(vs_transform_max_corner_displacement(&corr, W, H) == 0.0, "... which moves no corner", lag, i);
        }
    }
}

int main() {
    const int N = 24;
    for (int smoother : {1, 0})
        for (int lag : {0, 1, 4, N + 6}) {
            const vs_stabilizer_params p = params(lag, smoother);
            char what[96];
            for (double gain : {3.0, 40.0, 400.0}) {
                snprintf(what, sizeof what, "smoother %d lag %d gain %g", smoother, lag, gain);
                no_cut_is_stab_step(what, p, motions(N, gain, 17));
            }
            std::vector<Frame> f = motions(N, 40.0, 29);                  // failed alignments: the first two frames, a run in the middle, the last two
            for (int i : {0, 1, 9, 10, 11, N - 2, N - 1}) f[(size_t)i].ok = false;
            snprintf(what, sizeof what, "smoother %d lag %d: failed alignments", smoother, lag);
            no_cut_is_stab_step(what, p, f);
            f = motions(N, 5.0, 37);                                      // measurements with a NaN / an infinity
            f[5].meas.TX = std::nan(""); f[6].ok = false; f[15].meas.A = std::nan(""); f[16].meas.TY = INFINITY; f[17].ok = false;
            snprintf(what, sizeof what, "smoother %d lag %d: NaN", smoother, lag);
            no_cut_is_stab_step(what, p, f);
        }
    for (int smoother : {1, 0})
        for (int lag : {0, 1, 4})
            for (int at : {1, 7, 12})
                for (bool failed : {false, true}) one_cut(lag, smoother, at, failed);

    // By hand: smoother off, lag 1, translations of 10 along x.  accum after frame i + 1 finalises frame i's measurement: 0.9 * (accum + 10).
    {
        const vs_stabilizer_params p = params(1, 0);
        Side s(p);
        const vs_transform m{0, 0, 10, 0};
        vs_transform corr;
        double want = 0.0;
        for (int i = 0; i < 6; i++) {
            const bool cut = i == 3;
            const bool fin = vsi::stab_step_cut(m, true, cut, W, H, s.p, s.smoother, s.measurements, s.ok, s.cuts, s.accum, &corr);
            expect(fin == (i >= 1), "lag 1: finalised from the second frame on", i);
            if (i >= 1) want = (i - 1 == 3) ? 0.0 : (want + 10.0) * p.min_decay;     // frame 4 finalises the cut frame 3: the identity
            expect(s.accum.TX == want && s.accum.TY == 0.0, "hand-worked accum", i);
            if (i == 3) expect(s.ok.back() == 0 && s.measurements.back().TX == 0.0, "the cut frame: ok 0, the identity queued", i);
        }
        expect(want == 10.0 * p.min_decay, "after the cut the path starts from zero", 0);
    }
    if (failures) { printf("%d FAILURE(S)\n", failures); return 1; }
    printf("ALL PASS\n");
    return 0;
}
