// vs_align_plan.hpp -- the parts of the aligner's run path (vs_engine.hip) that are pure functions of integers: the level table, how a batch is
// cut into chunks, which frames of a chunk are keyframes and which form pairs, the fused solver's launch plan, and the conversion of a pair's
// device state into the API's result.  Host only, no HIP: tests/cpp/align_plan_test.cpp builds it with plain g++.
#pragma once

#include "vs_internal.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

// Internal linkage on purpose: PairState, PairDesc and GnParams are parameter types of vs_engine.hip's kernels, whose symbols live in that
// translation unit's unnamed namespace; the header is part of that unit (and of its test), not an interface between units: a second
// includer would get its own struct types and its own copy of solver_knobs().
#ifndef VS_ALIGN_PLAN_UNIT
#error "vs_align_plan.hpp belongs to vs_engine.hip and tests/cpp/align_plan_test.cpp only (they define VS_ALIGN_PLAN_UNIT)"
#endif
namespace {

constexpr int kMaxLevels = 16;
// on-device selection keeps (abs_delta,index) u32 + a u16 rank table per tile in LDS: 6 B x tiles <= 160 KB less
// the static part; index fits 16 bits; a thread's chunk fits a 32-bit mask
constexpr int kSelectCap = 26000;
constexpr size_t kLdsBound = 150 * 1024;   // dynamic LDS the fused solver asks for at most (next to its static part)

// ---- level table (alignment.cpp:155-204) -----------------------------------------------------------
struct LevelDims {
    int w, h, ts, tx, ty, nt, nsel;
    size_t img_off;   // bytes from the start of a frame's pyramid
    size_t lm_off;    // u16 elements from the start of a frame's arg-max table (x-set); y-set follows at +2*nt
    size_t jac_off;   // f32 elements from the start of a frame's Jacobian table (x-set); y-set at +4*nt
};
struct LevelTable {
    int levels = 0;
    LevelDims L[kMaxLevels];
    size_t pyr_frame = 0, lm_frame = 0, jac_frame = 0;   // bytes / u16 elements / f32 elements per slot
    int nt_max = 0;
    // nsel follows the *current* params like the reference (alignment.cpp:464-465: both sets keep size * fraction)
    void set_fraction(float fraction) {
        for (int l = 0; l < levels; l++) L[l].nsel = (int)static_cast<size_t>((size_t)L[l].nt * fraction);
    }
};
// The table of a w x h frame, or the refusal of a size the pipeline does not take; *out is written on success only.
inline int build_levels(int w, int h, const vs_aligner_params& p, LevelTable* out) {
    int lv = 0, ww = w, hh = h;
    do { lv++; ww /= 2; hh /= 2; } while (ww >= p.pyramid_min_width && hh >= p.pyramid_min_height);
    // PhaseLevel = 2 is indexed unconditionally in the reference (alignment.cpp:227): < 3 levels is UB there
    if (lv < 3 || lv > kMaxLevels)
        return vsi::set_error(VS_ERR_UNSUPPORTED, "%dx%d with pyramid_min %dx%d gives %d pyramid levels; 3..%d supported", w, h,
                              p.pyramid_min_width, p.pyramid_min_height, lv, kMaxLevels);
    if (w > 65535 || h > 65535) return vsi::set_error(VS_ERR_UNSUPPORTED, "frame larger than 65535 (u16 keypoints)");
    LevelTable t{};
    t.levels = lv;
    size_t img = 0, lmo = 0, jo = 0;
    ww = w; hh = h;
    for (int i = 0; i < lv; i++) {
        if (i > 0) { ww /= 2; hh /= 2; }
        LevelDims& l = t.L[i];
        l.w = ww; l.h = hh;
        l.ts = vs_tile_size(ww, hh);
        if (ww < 4 || hh < 4 || (ww / l.ts) * (hh / l.ts) < 1)
            return vsi::set_error(VS_ERR_UNSUPPORTED, "pyramid level %d is %dx%d: levels below 4x4 are not supported", i, ww, hh);
        l.tx = ww / l.ts; l.ty = hh / l.ts; l.nt = l.tx * l.ty;
        l.img_off = img; img += ((size_t)ww * hh + 255) & ~(size_t)255;
        l.lm_off = lmo; lmo += (size_t)l.nt * 4;     // x-set (2*nt) + y-set (2*nt)
        l.jac_off = jo; jo += (size_t)l.nt * 8;      // x-set (4*nt) + y-set (4*nt)
        t.nt_max = std::max(t.nt_max, l.nt);
    }
    t.pyr_frame = img; t.lm_frame = (lmo + 63) & ~(size_t)63; t.jac_frame = (jo + 63) & ~(size_t)63;
    t.set_fraction(p.smallest_fraction);
    *out = t;
    return VS_OK;
}

// ---- chunk sizing --------------------------------------------------------------------------------
// Frames per chunk: chunking bounds device memory to ~6 GiB of pyramids per handle; clips travel whole.
inline int max_chunk_frames(size_t pyr_frame, int clip_len, int* max_chunk) {
    int m = (int)std::max<size_t>(2, std::min<size_t>(1024, ((size_t)6 << 30) / std::max<size_t>(1, pyr_frame)));
    if (clip_len > 0) {
        if (clip_len > m) return vsi::set_error(VS_ERR_UNSUPPORTED, "clips of %d frames exceed the %d-frame chunk", clip_len, m);
        m -= m % clip_len;
    }
    *max_chunk = m;
    return VS_OK;
}
// Frames per upload of a host-resident batch: vs_internal.hpp's rule, the stabilizer's too (vs_stab_plan.hpp)
using vsi::host_chunk_frames;
// An n-frame call in chunks of m frames: chunk k of chunk_count(n, m) covers the frames [off, off + len).
struct ChunkSpan { int off, len; };
inline int chunk_count(int n, int m) { return (n + m - 1) / m; }
inline ChunkSpan chunk_span(int n, int m, int k) { return ChunkSpan{k * m, std::min(m, n - k * m)}; }

// ---- frame bookkeeping of one chunk ----------------------------------------------------------------
struct PairDesc {
    int32_t tmpl_slot;   // slot of the even (non-keyframe) frame: ScalePyramid[NonKeyframeIndex]
    int32_t key_slot;    // slot of the odd (keyframe) frame:      ScalePyramid[KeyframeIndex]
};
// Frame i of the chunk sits in slot i + 1 (slot 0: the carry-over frame); its index in its sequence is g(i) = seq0 + i, or i mod clip_len
// when the batch is a set of independent clips (every clip starts its own sequence at 0).  Odd g: a keyframe (alignment.hpp:65-66).  A pair
// exists for frame i when g(i) >= 1: frames (g-1, g) = slots (i, i+1).
struct ChunkFrames {
    long long seq0 = 0;
    int clip_len = 0, n = 0;
    std::vector<int> pair_frame;                  // the chunk frame of pair q
    std::vector<std::pair<int, int>> key_runs;    // (first_odd, n_odd): the keyframes, as stride-2 progressions of chunk frames
    void assign(long long seq0_, int clip_len_, int n_) {
        seq0 = seq0_; clip_len = clip_len_; n = n_;
        pair_frame.clear(); key_runs.clear();
        pair_frame.reserve(n);
        for (int i = 0; i < n; i++) if (!first(i)) pair_frame.push_back(i);
        // clips of odd length restart the parity, so each is a run of its own
        const int run = clip_len > 0 && (clip_len & 1) ? clip_len : n;
        for (int r0 = 0; r0 < n; r0 += run) {
            const int r1 = std::min(n, r0 + run), first_odd = r0 + ((g(r0) & 1) ? 0 : 1);
            if (first_odd < r1) key_runs.emplace_back(first_odd, (r1 - first_odd + 1) / 2);
        }
    }
    long long g(int i) const { return clip_len > 0 ? (long long)(i % clip_len) : seq0 + i; }
    bool first(int i) const { return g(i) < 1; }              // alignment.cpp:231-234: first frame of a sequence
    int n_pairs() const { return (int)pair_frame.size(); }
    bool negate(int q) const { return g(pair_frame[q]) & 1; }   // CurrFrameIndex == KeyframeIndex: the phase start value changes sign
    PairDesc desc(int q) const {
        const int i = pair_frame[q];
        return negate(q) ? PairDesc{i, i + 1} : PairDesc{i + 1, i};
    }
};

// ---- the fused solver's launch plan ----------------------------------------------------------------
// per-pair solver state, device resident; copied back once per batch
struct PairState {
    double T[4];
    int32_t status;        // 1 running/aligned, 0 failed
    int32_t fail_reason;   // 2 max iters, 3 over displacement
    int32_t fail_level;
    int32_t pad;
    int32_t iterations[kMaxLevels];
    double condition[kMaxLevels];
    double level_T[kMaxLevels][4];   // the estimate each level ended on (vs_align_info::level_transform)
};

struct GnParams {
    double threshold, max_displacement;
    int max_iters;
    int pipeline;   // 1: the one-barrier iteration loop on the LDS-resident level (latency mode, few pairs in flight)
    int stall_helpers;   // test hook (VS_GN_STALL_HELPERS=1): helpers never report back, the leader's bounded wait must expire
    int sel_depth_cap;   // test hook (VS_GN_SELECT_DEPTH=k > 0): the on-device introselect gets k partition rounds instead of 2 lg n, so
                         // ordinary frames take the "libstdc++ would have heap-selected" exit (fail_reason 100 -> host redo)
    int sel_stable;      // VS_SELECT_STABLE: smallest by (abs_delta, tile index), survivors in tile order (stable_select)
};

// The solver reads one compact record per selected point (vs_engine.hip pair_recs): float4 j | u32 xy | f32 tv | f32 r0, both point sets
constexpr size_t kPointRecBytes = 16 + 4 + 4 + 4;
inline size_t recs_pair_bytes(int nt_max) { return (size_t)2 * nt_max * kPointRecBytes; }

// latency mode: the descriptors of a small launch travel in the kernel arguments (no upload in front of the launch)
constexpr int kDirectMaxPairs = 16;
constexpr int kCoopGroup = 16;         // workgroups per pair in latency mode (1080p: 8 and 16 alike; 4K: 16 is 3 % faster)
constexpr int kCoopMaxGroup = 16;
constexpr int kCoopMaxPairs = 128;     // helpers for launches of at most this many pairs (16 per pair up to 16 pairs, then as many as keep the launch within one workgroup per CU)
constexpr int kChipCUs = 256;
constexpr int kCoopMinTiles = 4096;    // levels with at least this many tiles are shared
constexpr int kCoResidentMaxTiles = 128 * 256;          // introselect_block_g: 128 elements per thread (and <= kSelectCap)
constexpr size_t kCoResidentDynMax = 32 * 1024;        // dynamic LDS of the small-footprint build; larger levels select on global scratch
constexpr int kSmallWgTiles = 26000;     // largest level handled by the 512-thread kernels (<= kSelectCap <= 64 * 512)
constexpr int kPipelineMaxPairs = 128;   // half the CUs
// the three builds of the per-pair kernels (vs_engine.hip: nt512, nt1024, nt256v) and their workgroup sizes
enum { kBuild512 = 0, kBuild1024 = 1, kBuild256v = 2, kBuilds = 3 };
constexpr int kBuildThreads[kBuilds] = {512, 1024, 256};
inline int wg_build(int nt) { return nt <= kSmallWgTiles ? kBuild512 : kBuild1024; }

// The environment knobs of the solver launch, read once per process (the tests that set them run in child processes).
struct SolverKnobs {
    int pipeline = -1;        // VS_GN_PIPELINE=0|1 overrides the pipelined-loop rule
    int stall_helpers = 0;    // VS_GN_STALL_HELPERS (GnParams::stall_helpers)
    int select_depth = 0;     // VS_GN_SELECT_DEPTH (GnParams::sel_depth_cap)
    int helpers = -1;         // VS_GN_HELPERS=k: workgroups per pair where helpers apply
    int coresident = -1;      // VS_GN_CORESIDENT=0|1 overrides the small-footprint rule (1: every launch, helpers off)
    bool poll = true;         // VS_GN_POLL=0: the host sleeps in the runtime instead of spinning on the result words
};
inline const SolverKnobs& solver_knobs() {
    static const auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    static const SolverKnobs knobs{num("VS_GN_PIPELINE", -1), num("VS_GN_STALL_HELPERS", 0), num("VS_GN_SELECT_DEPTH", 0), num("VS_GN_HELPERS", -1),
                                   num("VS_GN_CORESIDENT", -1), num("VS_GN_POLL", 1) != 0};
    return knobs;
}

struct SolverPlan {
    // Latency mode (a few pairs, device-side selection, identity start): no copies around the launch at all -- the descriptors travel in
    // the kernel arguments, the kernel starts from the identity itself and writes its result straight into the pinned host block the host
    // reads after the synchronisation.
    bool direct = false;
    bool use_host = false;   // selection on the host, level by level (VS_SELECT_STL_HOST, or a level beyond the on-device capacity): no fused launch
    GnParams gp{};
    size_t recs_pair = 0;
    // the fused launch (not use_host)
    int group = 1;           // workgroups per pair: the leader and its helpers (vs_engine.hip CoopCtrl)
    bool cores = false;      // the small-footprint build
    int build = kBuild512, threads = kBuildThreads[kBuild512];
    size_t dyn = 0;          // dynamic LDS
    size_t selbuf_pair = 0, selbuf_bytes = 0;   // small-footprint build: global selection scratch per pair, and the buffer wanted
};
inline SolverPlan plan_solver(const LevelTable& t, int n_pairs, int cap, const vs_aligner_params& p, int select_mode, int batch_mode,
                              int cu_count, bool coop_ok, const SolverKnobs& k) {
    SolverPlan s;
    const int nt_max = t.nt_max, levels = t.levels;
    s.direct = n_pairs <= kDirectMaxPairs && !p.phase_correlate && select_mode != VS_SELECT_STL_HOST && nt_max <= kSelectCap;
    s.use_host = select_mode == VS_SELECT_STL_HOST || nt_max > kSelectCap;
    s.recs_pair = recs_pair_bytes(nt_max);
    // The pipelined iteration loop shortens one pair's critical path at the price of a speculative sampling pass per level:
    // worth it while the launch does not fill the chip (the results are bit-identical either way).
    const int pipeline = k.pipeline >= 0 ? k.pipeline : (n_pairs <= kPipelineMaxPairs ? 1 : 0);
    s.gp = GnParams{p.threshold, p.max_displacement, p.max_iters, pipeline, k.stall_helpers, k.select_depth, select_mode == VS_SELECT_STABLE ? 1 : 0};
    if (s.use_host) return s;
    // selection arrays in LDS: 6 B per tile for one point set; 12 B when both sets fit, so that they are selected
    // side by side (introselect_dual) -- always for 1080p, for every level but the finest at 4K
    size_t dyn = (((size_t)nt_max * ((size_t)nt_max * 12 <= kLdsBound ? 12 : 6) + 15) & ~(size_t)15);
    // ... and room for the coarsest level's image if it fits next to the static LDS (the kernel stages it for the
    // Gauss-Newton iterations): 480x270 at 1080p / 4K with pyramid_min_width 256
    const size_t img_bytes = (size_t)t.L[levels - 1].w * t.L[levels - 1].h + 8;
    if (img_bytes <= kLdsBound) dyn = std::max(dyn, (img_bytes + 15) & ~(size_t)15);
    // ... and its selection arrays behind the image, so that the level's sparse_warpdiff samples from LDS too
    const size_t both = ((img_bytes + 15) & ~(size_t)15) + (size_t)t.L[levels - 1].nt * 12;
    if (both <= kLdsBound) dyn = std::max(dyn, (both + 15) & ~(size_t)15);
    dyn = std::max<size_t>(dyn, 512);       // (tiny levels: the wave-level selection rounds use 128 bytes behind the keys as scratch)
    // latency mode: helper workgroups for the large levels of a pair
    if (coop_ok && n_pairs <= kCoopMaxPairs && t.L[0].nt >= kCoopMinTiles)
        s.group = k.helpers >= 0 ? std::max(1, std::min(k.helpers, kCoopMaxGroup)) : std::max(1, std::min(kCoopGroup, cu_count / n_pairs));
    // full batches of a handle in VS_BATCH_SHARED mode: the small-footprint build (shares CUs with whatever else is
    // running, e.g. the previous clip's warp launch)
    s.build = wg_build(nt_max);
    s.cores = s.build == kBuild512 && nt_max <= kCoResidentMaxTiles &&
              (k.coresident >= 0 ? k.coresident != 0 : (batch_mode == VS_BATCH_SHARED && n_pairs >= vsi::kSharedMinPairs));
    s.selbuf_pair = (((size_t)nt_max * 6 + 255) & ~(size_t)255);
    if (s.cores) {
        s.build = kBuild256v;
        s.group = 1;
        dyn = 16;
        bool need_global = false;
        for (int l = 0; l < levels; l++) {
            const size_t nt = (size_t)t.L[l].nt;
            const size_t need = ((nt <= 32 * (size_t)(kBuildThreads[kBuild256v] / 2) && nt * 12 <= kCoResidentDynMax ? nt * 12 : nt * 6) + 15) & ~(size_t)15;
            if (need <= kCoResidentDynMax) dyn = std::max(dyn, need); else need_global = true;
        }
        dyn = std::max<size_t>(dyn, 512);
        // (the kernel takes a non-null scratch pointer as "LDS block sized per level": always passed in this mode)
        s.selbuf_bytes = need_global ? s.selbuf_pair * (size_t)std::max(cap, n_pairs) : 256;
    }
    s.threads = kBuildThreads[s.build];
    s.dyn = dyn;
    return s;
}

// ---- result conversion -------------------------------------------------------------------------------
// The state a pair ended in -> the API's record, transform and flag of its frame (`inf` zeroed by the caller but for `levels`); g: the
// frame's sequence index.  Returns the pair's Gauss-Newton iterations.
inline int convert_result(const PairState& st, long long g, const LevelTable& t, vs_align_info* inf, vs_transform* out, int32_t* status) {
    int iterations = 0;
    inf->status = st.status; inf->fail_reason = st.fail_reason; inf->fail_level = st.fail_level;
    for (int l = 0; l < t.levels; l++) {
        inf->iterations[l] = st.iterations[l]; inf->condition[l] = st.condition[l]; iterations += st.iterations[l];
        if (st.iterations[l] > 0) {      // the level was reached (a level always runs at least one iteration)
            inf->selected_x[l] = t.L[l].nsel; inf->selected_y[l] = t.L[l].nsel;      // alignment.cpp:464-465: both sets keep size * fraction
            inf->level_transform[l] = vs_transform{st.level_T[l][0], st.level_T[l][1], st.level_T[l][2], st.level_T[l][3]};
        }
    }
    vs_transform tr{st.T[0], st.T[1], st.T[2], st.T[3]};
    if (st.status == 1) {
        if ((g & 1) == 0) tr = vs_transform_inverse(&tr);   // alignment.cpp:690-693
        *status = 1;
    }
    // on failure the reference returns false with `transform` left at the estimate it had reached
    // (alignment.cpp:661-667,674-677: no level rescale, no inversion) -- and VideoStabilizer feeds that value to
    // the smoother all the same (stabilizer.cpp:18-44), so it is part of the observable behaviour
    *out = tr;
    return iterations;
}

}  // namespace
