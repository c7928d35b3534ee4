// The integer half of the stabilizer's run path (video_stabilizer_amd/csrc/vs_stab_plan.hpp: the knobs, the route of a call, the depths of the
// look-ahead passes, scratch groups and warp runs) and the parameter ranges of vs_internal.hpp, against values worked out by hand from the
// rules as vs_stabilizer.hip had them in stab_run and stab_chunk, and against restatements written here.  Host only: built with the address
// and undefined-behaviour sanitizers together with csrc/vs_host.cpp (tests/test_stab_plan_cpp.py).
#include "../../video_stabilizer_amd/csrc/vs_stab_plan.hpp"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace vsi::stab;
using Kind = StabRoute::Kind;

static int failures = 0;
static void expect(bool cond, const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
    if (!cond) { if (failures < 40) printf("FAIL %s (%lld %lld %lld %lld)\n", what, a, b, c, d); failures++; }
}

// ---- knobs -------------------------------------------------------------------------------------------
static const char* env_name = nullptr;    // the one variable that is set, and its value (null: unset)
static const char* env_value = nullptr;
static const char* fake_env(const char* name) { return env_name && strcmp(name, env_name) == 0 ? env_value : nullptr; }

static const StabKnobs kDefaults{true, true, VS_BATCH_EXCLUSIVE, 0, 4};
static bool same(const StabKnobs& a, const StabKnobs& b) {
    return a.overlap == b.overlap && a.prefetch == b.prefetch && a.cv_solver == b.cv_solver && a.groups == b.groups && a.max_time_chunks == b.max_time_chunks;
}
static void knob_parsing() {
    expect(VS_BATCH_EXCLUSIVE == 0 && VS_BATCH_SHARED == 1, "the solver builds' numbers");
    env_name = nullptr;
    expect(same(stab_knobs_from(fake_env), kDefaults), "nothing set: overlap, prefetch, the exclusive build, default groups, 4 time chunks");
    const char* const values[6] = {nullptr, "0", "1", "2", "-3", "abc"};
    //                                unset  0  1  2 -3 abc
    const int want_switch[6] =       {1,     0, 1, 1, 1, 0};      // unset: on; else atoi != 0
    const int want_solver[6] =       {0,     0, 1, 0, 0, 0};      // VS_BATCH_SHARED only when atoi equals it
    const int want_groups[6] =       {0,     0, 1, 2, 0, 0};      // atoi >= 1, else 0: the default
    const int want_chunks[6] =       {4,     4, 1, 2, 4, 4};      // atoi >= 1, else 4
    for (int v = 0; v < 6; v++) {
        env_value = values[v];
        StabKnobs w = kDefaults;
        env_name = "VS_STAB_OVERLAP"; w.overlap = want_switch[v] != 0;
        expect(same(stab_knobs_from(fake_env), w), "VS_STAB_OVERLAP", v);
        w = kDefaults; env_name = "VS_STAB_PREFETCH"; w.prefetch = want_switch[v] != 0;
        expect(same(stab_knobs_from(fake_env), w), "VS_STAB_PREFETCH", v);
        w = kDefaults; env_name = "VS_STAB_CV_SOLVER"; w.cv_solver = want_solver[v];
        expect(same(stab_knobs_from(fake_env), w), "VS_STAB_CV_SOLVER", v);
        w = kDefaults; env_name = "VS_STAB_GROUPS"; w.groups = want_groups[v];
        expect(same(stab_knobs_from(fake_env), w), "VS_STAB_GROUPS", v);
        w = kDefaults; env_name = "VS_STAB_TIME_CHUNKS"; w.max_time_chunks = want_chunks[v];
        expect(same(stab_knobs_from(fake_env), w), "VS_STAB_TIME_CHUNKS", v);
    }
    env_name = nullptr;
    expect(&stab_knobs() == &stab_knobs(), "the process's knobs are one object, read once");
}

// ---- the route table ---------------------------------------------------------------------------------
constexpr int kLanczos2 = VS_WARP_LANCZOS2, kCv = VS_WARP_BILINEAR_CV;
constexpr size_t kFrame = (size_t)64 * 48 * 3;   // 9216 bytes: 64 x 48, 8-bit
static RouteIn host_call(int n, int clip_len, size_t ingest) { return RouteIn{VS_MEM_HOST, n, clip_len, 64, 48, kFrame, true, false, kCv, ingest}; }
static RouteIn device_call(int n, int clip_len, int warp_mode) { return RouteIn{VS_MEM_DEVICE, n, clip_len, 64, 48, kFrame, true, false, warp_mode, (size_t)192 << 20}; }
static void is_route(const char* what, const RouteIn& in, const StabKnobs& k, Kind kind, int step = 0, int solver = -1, int defer = -1) {
    const StabRoute r = pick_route(in, k);
    expect(r.kind == kind, what, r.kind, kind);
    if (kind != StabRoute::Plain) expect(r.step == step, what, r.step, step);
    if (solver >= 0) expect(r.solver_mode == solver, what, r.solver_mode, solver);
    if (defer >= 0) expect((int)r.defer == defer, what, r.defer, defer);
    expect(r.prefetch == k.prefetch, "prefetch follows the knob");
}
static void route_table() {
    const StabKnobs d = kDefaults;
    StabKnobs k;
    // host batches: the pipeline from one frame more than the upload chunk on
    is_route("host, one frame", host_call(1, 0, 30 * kFrame), d, StabRoute::Plain);
    is_route("host, n equal to the chunk", host_call(30, 0, 30 * kFrame), d, StabRoute::Plain);
    is_route("host, n = chunk + 1", host_call(31, 0, 30 * kFrame), d, StabRoute::HostPipelined, 30);
    is_route("host, an upload budget below one frame: 4 frames", host_call(5, 0, kFrame - 1), d, StabRoute::HostPipelined, 4);
    is_route("host, ... and 4 frames fit one chunk", host_call(4, 0, kFrame - 1), d, StabRoute::Plain);
    is_route("host, clips of 7 in a chunk of 30: 28", host_call(35, 7, 30 * kFrame), d, StabRoute::HostPipelined, 28);
    is_route("host, clips longer than the byte-derived chunk travel whole", host_call(80, 40, 30 * kFrame), d, StabRoute::HostPipelined, 40);
    // device-resident clip batches: groups
    is_route("8 clips x 60, Lanczos2", device_call(480, 60, kLanczos2), d, StabRoute::ClipGroups, 120, VS_BATCH_SHARED, 0);
    is_route("8 clips x 60, fixed-point bilinear", device_call(480, 60, kCv), d, StabRoute::ClipGroups, 240, VS_BATCH_EXCLUSIVE, 0);
    k = d; k.cv_solver = VS_BATCH_SHARED;
    is_route("... with VS_STAB_CV_SOLVER=1", device_call(480, 60, kCv), k, StabRoute::ClipGroups, 120, VS_BATCH_SHARED, 0);
    is_route("VS_STAB_CV_SOLVER leaves a Lanczos2 handle alone", device_call(480, 60, kLanczos2), k, StabRoute::ClipGroups, 120, VS_BATCH_SHARED, 0);
    k = d; k.groups = 8;
    is_route("VS_STAB_GROUPS=8", device_call(480, 60, kLanczos2), k, StabRoute::ClipGroups, 60, VS_BATCH_SHARED, 0);
    is_route("VS_STAB_GROUPS=8, fixed-point bilinear", device_call(480, 60, kCv), k, StabRoute::ClipGroups, 60, VS_BATCH_EXCLUSIVE, 0);
    is_route("one clip", device_call(60, 60, kLanczos2), d, StabRoute::Plain);
    is_route("clips of one frame", device_call(8, 1, kLanczos2), d, StabRoute::Plain);
    is_route("n is no whole number of clips", device_call(481, 60, kLanczos2), d, StabRoute::Plain);
    is_route("2 clips x 3: the group would take every clip", device_call(6, 3, kLanczos2), d, StabRoute::Plain);
    // one long device-resident clip: time chunks
    is_route("n = 95", device_call(95, 0, kLanczos2), d, StabRoute::Plain);
    is_route("n = 96, Lanczos2", device_call(96, 0, kLanczos2), d, StabRoute::TimeChunks, 48, VS_BATCH_SHARED, 1);
    is_route("n = 96, fixed-point bilinear: a chunk of 120 is the call", device_call(96, 0, kCv), d, StabRoute::Plain);
    is_route("n = 480, Lanczos2", device_call(480, 0, kLanczos2), d, StabRoute::TimeChunks, 120, VS_BATCH_SHARED, 1);
    is_route("n = 480, fixed-point bilinear", device_call(480, 0, kCv), d, StabRoute::TimeChunks, 120, VS_BATCH_EXCLUSIVE, 1);
    k = d; k.max_time_chunks = 8;
    is_route("n = 480, VS_STAB_TIME_CHUNKS=8, Lanczos2", device_call(480, 0, kLanczos2), k, StabRoute::TimeChunks, 60, VS_BATCH_SHARED, 1);
    // the switches
    k = d; k.overlap = false;
    is_route("VS_STAB_OVERLAP=0, clips", device_call(480, 60, kLanczos2), k, StabRoute::Plain);
    is_route("VS_STAB_OVERLAP=0, one clip", device_call(480, 0, kLanczos2), k, StabRoute::Plain);
    is_route("VS_STAB_OVERLAP=0, host: still pipelined", host_call(31, 0, 30 * kFrame), k, StabRoute::HostPipelined, 30);
    RouteIn in = device_call(480, 60, kLanczos2);
    in.dense = false;
    is_route("pitched device frames, clips", in, d, StabRoute::Plain);
    in = device_call(480, 0, kLanczos2); in.dense = false;
    is_route("pitched device frames, one clip", in, d, StabRoute::Plain);
    in = device_call(480, 60, kLanczos2); in.lens_on = true;
    is_route("lens correction, device clips", in, d, StabRoute::Plain);
    in = device_call(480, 0, kCv); in.lens_on = true;
    is_route("lens correction, one device clip", in, d, StabRoute::Plain);
    in = host_call(31, 0, 30 * kFrame); in.lens_on = true;
    is_route("lens correction, host: still pipelined", in, d, StabRoute::HostPipelined, 30);
    k = d; k.prefetch = false;
    is_route("VS_STAB_PREFETCH=0 reaches the route", device_call(480, 60, kLanczos2), k, StabRoute::ClipGroups, 120, VS_BATCH_SHARED, 0);
    is_route("VS_STAB_PREFETCH=0 reaches the route, time chunks", device_call(480, 0, kCv), k, StabRoute::TimeChunks, 120, VS_BATCH_EXCLUSIVE, 1);
}

// ---- invariants over a sweep ---------------------------------------------------------------------------
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }
static int pick(std::initializer_list<int> v) { return v.begin()[rnd() % v.size()]; }
static RouteIn random_call() {
    RouteIn in{};
    in.mem = rnd() % 3 ? VS_MEM_DEVICE : VS_MEM_HOST;
    in.clip_len = rnd() % 2 ? 0 : pick({1, 2, 3, 7, 17, 33, 60, 100});
    in.n = in.clip_len > 0 && rnd() % 8 ? in.clip_len * pick({1, 2, 3, 4, 5, 8, 9, 16, 31}) : pick({1, 2, 3, 4, 5, 47, 48, 95, 96, 97, 119, 120, 121, 191, 192, 480, 481, 1000, 5000});
    in.w = rnd() % 16 ? pick({64, 161, 1920, 3840}) : 0;
    in.h = rnd() % 16 ? pick({48, 121, 1080, 2160}) : 0;
    in.frame_bytes = (size_t)in.w * in.h * 3 * (rnd() % 2 ? 1 : 2);
    in.dense = rnd() % 8 != 0;
    in.lens_on = rnd() % 8 == 0;
    in.warp_mode = pick({VS_WARP_LANCZOS2, VS_WARP_BILINEAR, VS_WARP_LANCZOS2_FAST, VS_WARP_LANCZOS2_SEP, VS_WARP_BILINEAR_CV});
    in.ingest_bytes = (size_t)pick({1, 9215, 150000, 1000000}) * (rnd() % 2 ? 1 : 192);
    return in;
}
static StabKnobs random_knobs() {
    return StabKnobs{rnd() % 8 != 0, rnd() % 2 != 0, rnd() % 2 ? VS_BATCH_SHARED : VS_BATCH_EXCLUSIVE, pick({0, 0, 1, 2, 3, 8}), pick({4, 4, 1, 2, 8})};
}
static void sweep() {
    int seen[4] = {0, 0, 0, 0};
    for (int it = 0; it < 6000; it++) {
        const RouteIn in = random_call();
        const StabKnobs k = random_knobs();
        const StabRoute r = pick_route(in, k);
        seen[r.kind]++;
        const int n = in.n, len = in.clip_len;
        expect(r.step >= 1, "a step has frames", r.step);
        const int steps = (n + r.step - 1) / r.step;
        long long covered = 0;
        for (int s = 0; s < steps; s++) covered += std::min(r.step, n - s * r.step);
        expect(covered == n && (long long)(steps - 1) * r.step < n, "the steps cover the call, none of them empty", n, r.step);
        const int solver = in.warp_mode == VS_WARP_BILINEAR_CV ? k.cv_solver : VS_BATCH_SHARED;
        // the stabilizer's former expression for the upload chunk equals the shared rule without a chunk limit
        int old_chunk = (int)std::max<size_t>(4, in.ingest_bytes / std::max<size_t>(1, in.frame_bytes));
        if (len > 0) old_chunk = std::max(len, old_chunk - old_chunk % len);
        expect(old_chunk == vsi::host_chunk_frames(INT_MAX, in.ingest_bytes, in.frame_bytes, len), "one host-chunk rule", old_chunk, len);
        if (len > 0) expect(old_chunk % len == 0 && old_chunk >= len, "an upload holds whole clips", old_chunk, len);
        expect(old_chunk >= 4 || len > 0, "an upload holds at least 4 frames", old_chunk);
        // the preconditions, restated
        const bool host_pipe = in.mem == VS_MEM_HOST && n > 1 && in.w > 0 && in.h > 0 && n > old_chunk;
        const bool dev = k.overlap && !in.lens_on && in.mem == VS_MEM_DEVICE && in.w > 0 && n > 1 && in.dense;
        const bool clips = dev && len >= 2 && n % len == 0 && n / len >= 2;
        const bool long_clip = dev && len == 0 && n >= 96;
        expect((r.kind == StabRoute::HostPipelined) == host_pipe, "the pipeline: host frames, more than one upload", n, old_chunk);
        if (host_pipe) expect(r.step == old_chunk, "... in uploads of the chunk", r.step, old_chunk);
        if (!clips) expect(r.kind != StabRoute::ClipGroups, "no groups unless the preconditions hold", n, len);
        if (!long_clip) expect(r.kind != StabRoute::TimeChunks, "no time chunks unless the preconditions hold", n, len);
        if (!host_pipe && !clips && !long_clip) expect(r.kind == StabRoute::Plain, "the plain route whenever the preconditions fail", n, len);
        if (r.kind == StabRoute::ClipGroups) {
            const int max_groups = k.groups ? k.groups : (solver == VS_BATCH_EXCLUSIVE ? 2 : 4);
            expect(r.step % len == 0 && r.step < n, "a group is whole clips, and not all of them", r.step, len);
            expect(steps <= max_groups, "at most max_groups groups", steps, max_groups);
            // (the last group is what is left over; every other one is a full step)
            expect(r.step / len * (len - 1) >= vsi::kSharedMinPairs, "a full group holds at least kSharedMinPairs pairs", r.step, len);
            expect(!r.defer && r.solver_mode == solver, "groups: nothing deferred, the solver build of the warp mode", r.solver_mode);
        }
        if (r.kind == StabRoute::TimeChunks) {
            expect(r.step >= (solver == VS_BATCH_EXCLUSIVE ? 120 : 48) && r.step < n, "a time chunk has 48 / 120 frames at least, by solver build", r.step, solver);
            expect(steps <= k.max_time_chunks, "at most max_time_chunks chunks", steps, k.max_time_chunks);
            expect(r.defer && r.solver_mode == solver, "time chunks: queued frames stay deferred", r.solver_mode);
        }
        if (r.kind == StabRoute::Plain) expect(r.step == n, "the plain route: one step", r.step, n);
        expect(r.prefetch == k.prefetch, "prefetch follows the knob");
    }
    expect(seen[0] > 300 && seen[1] > 300 && seen[2] > 300 && seen[3] > 300, "the sweep reaches every route", seen[0], seen[1], seen[2], seen[3]);
}

// ---- plan_passes ---------------------------------------------------------------------------------------
static void pass_depths() {
    PassConfig on;
    on.border_fill = 3; on.deblur = 2; on.denoise = 5; on.deflicker = 4; on.rolling.readout = 0.5;
    on.fill_blend = vs_fill_blend_params{2, 1};
    for (int mode : {VS_WARP_LANCZOS2, VS_WARP_BILINEAR, VS_WARP_LANCZOS2_FAST, VS_WARP_LANCZOS2_SEP, VS_WARP_BILINEAR_CV}) {
        const PassPlan z = plan_passes(on, 0, mode);
        expect(z.fill == 0 && z.deblur == 0 && z.denoise == 0 && z.deflicker == 0 && z.rolling == 0 && !z.blend_on && !z.want_sums, "lag 0: every depth is zero", mode);
        const int cv = mode == VS_WARP_BILINEAR_CV;
        const PassPlan a = plan_passes(on, 1, mode);
        expect(a.fill == cv && a.deblur == 1 && a.denoise == 1 && a.deflicker == 1 && a.rolling == 1, "lag 1 caps every depth", mode);
        const PassPlan b = plan_passes(on, 3, mode);
        expect(b.fill == 3 * cv && b.deblur == 2 && b.denoise == 3 && b.deflicker == 3 && b.rolling == 1, "lag 3: min(setting, lag)", mode);
        const PassPlan c = plan_passes(on, 30, mode);
        expect(c.fill == 3 * cv && c.deblur == 2 && c.denoise == 5 && c.deflicker == 4 && c.rolling == 1, "a long lag: the settings", mode);
        expect(c.blend_on == (cv != 0) && c.want_sums == (cv != 0), "no fill, no blend, outside VS_WARP_BILINEAR_CV", mode);
    }
    const PassPlan off = plan_passes(PassConfig{}, 30, VS_WARP_BILINEAR_CV);
    expect(off.fill == 0 && off.deblur == 0 && off.denoise == 0 && off.deflicker == 0 && off.rolling == 0 && !off.blend_on && !off.want_sums, "a fresh handle runs no pass");
    // the rolling-shutter list: min(1, lag) if and only if the readout is not zero
    for (int lag : {0, 1, 7}) {
        PassConfig c;
        c.rolling.readout = -1.0;  expect(plan_passes(c, lag, VS_WARP_LANCZOS2).rolling == (lag > 0), "readout -1", lag);
        c.rolling.readout = 1e-300; expect(plan_passes(c, lag, VS_WARP_LANCZOS2).rolling == (lag > 0), "readout 1e-300", lag);
        c.rolling.readout = 0.0;   expect(plan_passes(c, lag, VS_WARP_LANCZOS2).rolling == 0, "readout 0: off", lag);
        c.rolling.readout = -0.0;  expect(plan_passes(c, lag, VS_WARP_LANCZOS2).rolling == 0, "readout -0: off", lag);
    }
    // blend_on and want_sums over (feather > 0, match), with the fill on and off
    const struct { int feather, match; bool blend, sums; } rows[4] = {{0, 0, false, false}, {3, 0, true, false}, {0, 1, true, true}, {3, 1, true, true}};
    for (const auto& row : rows) {
        PassConfig c;
        c.fill_blend = vs_fill_blend_params{row.feather, row.match};
        c.border_fill = 2;
        const PassPlan with = plan_passes(c, 4, VS_WARP_BILINEAR_CV);
        expect(with.fill == 2 && with.blend_on == row.blend && with.want_sums == row.sums, "the blend's truth table, fill on", row.feather, row.match);
        c.border_fill = 0;
        const PassPlan without = plan_passes(c, 4, VS_WARP_BILINEAR_CV);
        expect(without.fill == 0 && !without.blend_on && !without.want_sums, "fill off: no blend, no sums", row.feather, row.match);
        c.border_fill = 2;
        const PassPlan no_lag = plan_passes(c, 0, VS_WARP_BILINEAR_CV);
        expect(no_lag.fill == 0 && !no_lag.blend_on && !no_lag.want_sums, "fill set, lag 0: no blend, no sums", row.feather, row.match);
    }
}

// ---- scratch groups and warp runs -----------------------------------------------------------------------
static void groups_and_runs() {
    expect(scratch_group(10, 99, 100) == 1, "a budget below one frame: one frame");
    expect(scratch_group(10, 0, 100) == 1, "a budget of 0: one frame");
    expect(scratch_group(10, 100, 100) == 1 && scratch_group(10, 199, 100) == 1 && scratch_group(10, 200, 100) == 2, "exact multiples");
    expect(scratch_group(10, 999, 100) == 9 && scratch_group(10, 1000, 100) == 10 && scratch_group(10, 1001, 100) == 10, "up to the run");
    expect(scratch_group(10, (size_t)256 << 20, 100) == 10, "a budget above the run: the run");
    expect(scratch_group(1, 0, 100) == 1 && scratch_group(1, (size_t)256 << 20, 1) == 1, "a run of one");
    expect(scratch_group(43, (size_t)256 << 20, (size_t)1920 * 1080 * 3) == 43 && scratch_group(44, (size_t)256 << 20, (size_t)1920 * 1080 * 3) == 43,
           "256 MB: forty-three 1080p windows");

    const size_t fb = 16;
    std::vector<uint8_t> batch(8 * fb), own_a(fb), own_b(fb);
    const vs_transform t{0, 0, 0, 0};
    auto job = [&](const uint8_t* src, int i) { return Job{src, t, i, nullptr}; };
    std::vector<Job> one = {job(batch.data(), 0)};
    expect(run_end(one, 0, fb) == 1, "a single job");
    std::vector<Job> all;
    for (int i = 0; i < 8; i++) all.push_back(job(batch.data() + i * fb, i));
    expect(run_end(all, 0, fb) == 8 && run_end(all, 3, fb) == 8 && run_end(all, 7, fb) == 8, "consecutive batch frames are one run");
    expect(run_end(all, 0, 2 * fb) == 1, "another frame size: no run");
    std::vector<Job> gap_i = {job(batch.data(), 0), job(batch.data() + fb, 1), job(batch.data() + 2 * fb, 3), job(batch.data() + 3 * fb, 4)};
    expect(run_end(gap_i, 0, fb) == 2 && run_end(gap_i, 2, fb) == 4, "a gap in i ends a run");
    std::vector<Job> gap_src = {job(batch.data(), 0), job(batch.data() + fb, 1), job(batch.data() + 3 * fb, 2), job(batch.data() + 4 * fb, 3)};
    expect(run_end(gap_src, 0, fb) == 2 && run_end(gap_src, 2, fb) == 4, "a gap in the sources ends a run");
    // frames queued by earlier calls lie in buffers of the handle's, then the batch's own frames follow
    std::vector<Job> owned = {job(own_a.data(), 0), job(own_b.data(), 1), job(batch.data(), 2), job(batch.data() + fb, 3), job(batch.data() + 2 * fb, 4)};
    expect(run_end(owned, 0, fb) == 1 && run_end(owned, 1, fb) == 2 && run_end(owned, 2, fb) == 5, "owned buffers are runs of one, then the batch frames");
    size_t runs = 0;
    for (size_t j = 0; j < owned.size(); j = run_end(owned, j, fb)) runs++;
    expect(runs == 3, "the runs tile the jobs", (long long)runs);
}

// ---- the parameter ranges ----------------------------------------------------------------------------------
static void ranges() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
    using namespace vsi;
    for (int v : {INT_MIN, -1, 0, 256, INT_MAX}) expect(!denoise_params_valid(vs_denoise_params{v}), "denoise strength outside 1 .. 255", v);
    for (int v : {1, 24, 255}) expect(denoise_params_valid(vs_denoise_params{v}), "denoise strength 1 .. 255", v);
    for (int v : {INT_MIN, -1, 0, 65, INT_MAX}) expect(!deflicker_params_valid(vs_deflicker_params{v}), "deflicker step outside 1 .. 64", v);
    for (int v : {1, 4, 64}) expect(deflicker_params_valid(vs_deflicker_params{v}), "deflicker step 1 .. 64", v);
    for (int v : {INT_MIN, -1, 0, 33, INT_MAX}) expect(!sharpen_params_valid(vs_sharpen_params{v}), "sharpen strength outside 1 .. 32", v);
    for (int v : {1, 16, 32}) expect(sharpen_params_valid(vs_sharpen_params{v}), "sharpen strength 1 .. 32", v);
    for (int step : {INT_MIN, 0, 1, 64, 65, INT_MAX})
        for (int thr : {INT_MIN, 0, 1, 255, 256, INT_MAX})
            expect(scene_params_valid(vs_scene_params{step, thr}) == (step >= 1 && step <= 64 && thr >= 1 && thr <= 255), "scene step 1 .. 64, threshold 1 .. 255", step, thr);
    expect(scene_params_valid(vs_scene_params{4, 32}), "the scene default");
    for (int f : {INT_MIN, -1, 0, 1, 6, 7, INT_MAX})
        for (int m : {INT_MIN, -1, 0, 1, 2, INT_MAX})
            expect(fill_blend_params_valid(vs_fill_blend_params{f, m}) == (f >= 0 && f <= 6 && (m == 0 || m == 1)), "feather 0 .. 6, match 0 or 1", f, m);
    for (double v : {-1.0, -0.5, -0.0, 0.0, 1e-300, 0.5, 1.0}) expect(rolling_params_valid(vs_rolling_params{v}), "readout -1 .. 1");
    for (double v : {std::nextafter(-1.0, -2.0), std::nextafter(1.0, 2.0), -inf, inf, nan, -nan}) expect(!rolling_params_valid(vs_rolling_params{v}), "readout outside -1 .. 1, or a NaN");

    expect(deblur_params_finite(2.0f, 4.0f), "the deblur default");
    expect(!deblur_params_finite(0.0f, 4.0f) && !deblur_params_finite(-1.0f, 4.0f) && !deblur_params_finite(fnan, 4.0f) && !deblur_params_finite(finf, 4.0f), "sensitivity: positive, finite");
    expect(deblur_params_finite(3.0e38f, 4.0f) && !deblur_params_finite(std::nextafter(3.0e38f, finf), 4.0f), "sensitivity up to 3e38");
    expect(!deblur_params_finite(2.0f, 0.0f) && !deblur_params_finite(2.0f, -1.0f) && !deblur_params_finite(2.0f, fnan) && !deblur_params_finite(2.0f, finf), "max_ratio: positive, finite");
    expect(deblur_params_finite(3.0e38f, 1.0e18f) && !deblur_params_finite(3.0e38f, std::nextafter(1.0e18f, finf)), "max_ratio up to 1e18");
    expect(deblur_params_finite(1.0f, 0x1p50f) && !deblur_params_finite(1.0f, std::nextafter(0x1p50f, finf)), "max_ratio^2 <= sensitivity * 2^100");
    expect(deblur_params_finite(0x1p-100f, 1.0f) && !deblur_params_finite(std::nextafter(0x1p-100f, 0.0f), 1.0f), "... from the sensitivity's side");
    expect(deblur_params_finite(0x1p6f, 1.0e18f) && deblur_params_finite(0x1p6f, 0x1p53f) && !deblur_params_finite(std::nextafter(0x1p6f, 0.0f), 0x1p53f),
           "max_ratio counts up to 2^53 only: 2^106 <= sensitivity * 2^100 from sensitivity 64 on");
}

int main() {
    knob_parsing();
    route_table();
    sweep();
    pass_depths();
    groups_and_runs();
    ranges();
    if (failures) { printf("%d FAILURES\n", failures); return 1; }
    printf("ALL PASS\n");
    return 0;
}
