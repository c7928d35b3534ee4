// vs_stab_plan.hpp -- the parts of the stabilizer's run path (vs_stabilizer.hip) that are pure functions of integers: the environment knobs,
// how a call is cut (the route), what the handle's setters set and how deep each look-ahead pass then looks, the scratch groups and the
// warp runs.  Host only, no HIP: tests/cpp/stab_plan_test.cpp builds it with plain g++.
#pragma once

#include "vs_internal.hpp"

#include <climits>
#include <cstdlib>
#include <vector>

namespace vsi {
namespace stab {

// ---- knobs ---------------------------------------------------------------------------------------------
// The environment knobs of the route, read together once per process (the tests that set them run in child processes).
struct StabKnobs {
    bool overlap, prefetch;    // VS_STAB_OVERLAP=0: device batches take the plain route; VS_STAB_PREFETCH=0: no alignment is started ahead of time
    int cv_solver;             // VS_STAB_CV_SOLVER=1: the small-footprint solver build beside the fixed-point bilinear warp too (an A/B)
    int groups;                // VS_STAB_GROUPS: clip groups at most (0: the default, by solver build)
    int max_time_chunks;       // VS_STAB_TIME_CHUNKS: time chunks at most (4)
};
inline StabKnobs stab_knobs_from(const char* (*get)(const char*)) {
    const auto on = [&](const char* name) { const char* e = get(name); return e ? atoi(e) != 0 : true; };
    const auto at_least_1 = [&](const char* name, int unset) { const char* e = get(name); const int v = e ? atoi(e) : 0; return v >= 1 ? v : unset; };
    const char* const cv = get("VS_STAB_CV_SOLVER");
    return StabKnobs{on("VS_STAB_OVERLAP"), on("VS_STAB_PREFETCH"), cv && atoi(cv) == VS_BATCH_SHARED ? VS_BATCH_SHARED : VS_BATCH_EXCLUSIVE,
                     at_least_1("VS_STAB_GROUPS", 0), at_least_1("VS_STAB_TIME_CHUNKS", 4)};
}
inline const StabKnobs& stab_knobs() {
    static const StabKnobs knobs = stab_knobs_from([](const char* name) -> const char* { return getenv(name); });
    return knobs;
}

// ---- the route: how a call is cut ----------------------------------------------------------------------
// What of a call and its handle the decision reads.  dense: StabCall::dense(); ingest_bytes: vsi::ingest_chunk_bytes().
struct RouteIn { int mem, n, clip_len, w, h; size_t frame_bytes; bool dense, lens_on; int warp_mode; size_t ingest_bytes; };
// step: the frames of a sub-batch (Plain: the call's).  defer, solver_mode, prefetch: stab_run_overlapped's arguments, read by ClipGroups and
// TimeChunks only.
struct StabRoute { enum Kind { Plain, HostPipelined, ClipGroups, TimeChunks } kind; int step; bool defer; int solver_mode; bool prefetch; };
constexpr int kOverlapMinFrames = 96;            // one device-resident clip is cut in time from this many frames on
constexpr int kTimeChunkShared = 48, kTimeChunkExclusive = 120;   // ... into chunks of at least this many, by solver build
constexpr int kGroupsShared = 4, kGroupsExclusive = 2;             // clip groups at most, by solver build

inline StabRoute pick_route(const RouteIn& in, const StabKnobs& knobs) {
    const int n = in.n, clip_len = in.clip_len;
    // host-resident batches longer than one upload chunk run as a three-stage pipeline: upload / compute / download.  (The aligner's rule for
    // an upload; INT_MAX: the pipeline has no chunk limit of its own.)
    int chunk = 0;
    if (in.mem == VS_MEM_HOST && n > 1 && in.w > 0 && in.h > 0) chunk = host_chunk_frames(INT_MAX, in.ingest_bytes, in.frame_bytes, clip_len);
    // Device-resident clip batches (vs_stabilizer_process_clips, VS_MEM_DEVICE, dense frames): the clips are cut into groups and the
    // warps of group g go to a stream of their own, so that they run under the alignment of group g + 1 -- which then takes the
    // small-footprint solver build (VS_BATCH_SHARED: it shares CUs with the warp grid).  Every group goes through stab_run_impl
    // exactly as a process_clips call of its own would (clips are independent: stabilizer.cpp keeps no state across a reset), so
    // the grouping cannot change results.  VS_STAB_OVERLAP=0 turns it off.
    // (the solver build under the overlapped warps: the small-footprint one beside a Lanczos2 warp, which fills the CUs for longer than the
    // alignment pass takes; beside the fixed-point bilinear warp -- a quarter of the alignment pass -- the exclusive 512-thread build, whose
    // shorter solver chain is worth more than the shared CUs: 1080p x 480 frames 101 k -> 120 k frames/s, 4K x 240 21.1 k -> 34.3 k
    // (profiles/r05_stab_cv_solver.txt; VS_STAB_CV_SOLVER=1 selects the small build for an A/B))
    const int overlap_mode = in.warp_mode == VS_WARP_BILINEAR_CV ? knobs.cv_solver : VS_BATCH_SHARED;
    const int n_clips_all = clip_len > 0 ? n / clip_len : 0;
    // (lens correction on: the plain route.  The overlapped routes align the caller's uncorrected frames ahead of time, and their
    // deferred queue entries would point into batch_in, which the next sub-batch's corrected frames overwrite)
    const bool dense_dev = !in.lens_on && in.mem == VS_MEM_DEVICE && in.w > 0 && n > 1 && in.dense;
    int group_clips = 0;
    if (knobs.overlap && dense_dev && clip_len >= 2 && n_clips_all >= 2 && n == n_clips_all * clip_len) {
        // groups of at least kSharedMinPairs pairs (the small build's threshold), at most 4 groups (VS_STAB_GROUPS): every group boundary is a host
        // synchronisation and a latency-bound solver launch -- c5 (8 clips x 60 x 4K 10-bit) 17.3-18.1 k frames/s with 8 groups, 18.9-19.5 k with 4
        group_clips = std::max(1, (kSharedMinPairs + clip_len - 2) / (clip_len - 1));
        // (beside the fixed-point bilinear warp, with the exclusive solver build: 2 groups -- c5 27.8 k frames/s with 4 groups, 28.9 k with 2, 24.8 k with 8)
        const int max_groups = knobs.groups ? knobs.groups : (overlap_mode == VS_BATCH_EXCLUSIVE ? kGroupsExclusive : kGroupsShared);
        group_clips = std::max(group_clips, (n_clips_all + max_groups - 1) / max_groups);
        if (group_clips >= n_clips_all) group_clips = 0;
    }
    // ONE long device-resident clip: cut in time.  The batched form is n successive process calls, so the chunks are the same calls in the same
    // order.  Time chunks of >= 48 frames (the small solver build's threshold with room to spare), at most 4 of them (VS_STAB_TIME_CHUNKS:
    // 1080p x480 64 k frames/s with 8 chunks, 70 k with 6, 72 k with 4 or 3, 69-71 k with 2; profiles/r04_stab_long_clip.txt)
    // (with the exclusive solver build a chunk is a latency-bound chain of its own: chunks of >= 120 frames -- 4K x240 34.2 k frames/s in 4 chunks, 35.8 k in 2)
    int time_chunk = 0;
    if (knobs.overlap && dense_dev && clip_len == 0 && n >= kOverlapMinFrames)
        time_chunk = std::max(overlap_mode == VS_BATCH_EXCLUSIVE ? kTimeChunkExclusive : kTimeChunkShared, (n + knobs.max_time_chunks - 1) / knobs.max_time_chunks);
    if (time_chunk >= n) time_chunk = 0;
    if (chunk > 0 && n > chunk) return StabRoute{StabRoute::HostPipelined, chunk, false, overlap_mode, knobs.prefetch};
    if (group_clips > 0) return StabRoute{StabRoute::ClipGroups, group_clips * clip_len, false, overlap_mode, knobs.prefetch};
    if (time_chunk > 0) return StabRoute{StabRoute::TimeChunks, time_chunk, true, overlap_mode, knobs.prefetch};
    return StabRoute{StabRoute::Plain, std::max(1, n), false, overlap_mode, knobs.prefetch};
}

// ---- the passes: what the setters set, and how deep each pass looks ---------------------------------------
// What the handle's vs_stabilizer_set_* calls set.  A depth: following frames (0: off).
struct PassConfig {
    int border_fill = 0;           // vs_stabilizer_set_border_fill: candidates per output frame beyond the frame itself
    vs_fill_blend_params fill_blend{0, 0};   // vs_stabilizer_set_fill_blend
    int deblur = 0;                // vs_stabilizer_set_deblur: following frames a frame is deblurred from
    vs_deblur_params deblur_params{2.0f, 4.0f};
    int denoise = 0;               // vs_stabilizer_set_denoise: following frames a frame is averaged with
    vs_denoise_params denoise_params{24};
    int deflicker = 0;             // vs_stabilizer_set_deflicker: following frames in a frame's exposure window
    vs_deflicker_params deflicker_params{4};
    vs_rolling_params rolling{0.0};   // vs_stabilizer_set_rolling_shutter: readout 0: off
    int inpaint = 0;               // vs_stabilizer_set_inpaint: what no candidate covers in the output window is inpainted
    bool sharpen_on = false;       // vs_stabilizer_set_sharpen: NULL: off
    vs_sharpen_params sharpen{16};
    bool scene_on = false;         // vs_stabilizer_set_scene_cut: NULL: off
    vs_scene_params scene_params{4, 32};
    bool lens_on = false;          // vs_stabilizer_set_lens: NULL or the identity lens: off
    vs_lens_params lens{};
    int lens_w = 0, lens_h = 0;    // the frame size the lens was calibrated for; frames of another size are refused while the pass is on
    int out_w = 0, out_h = 0;      // vs_stabilizer_set_output_size: (0, 0) off -- the window is delivered; (-1, -1) the source frame's size; else the size
    int out_filter = VS_RESIZE_LINEAR;   // ... and the resize's filter
};
// What a call delivers: the crop window (w - 2 crop) x (h - 2 crop) as it is, or resized (vs_resize.hip) to the size the handle was given.
// resize: the pass runs -- a window that already has the requested size is delivered as it is, launch for launch the handle with the pass off.
struct Delivery { int w, h; bool resize; };
inline Delivery delivered_size(int w, int h, int crop, const PassConfig& c) {
    const int ow = w - 2 * crop, oh = h - 2 * crop;
    if (c.out_w == 0 && c.out_h == 0) return Delivery{ow, oh, false};
    const int dw = c.out_w < 0 ? w : c.out_w, dh = c.out_h < 0 ? h : c.out_h;
    return Delivery{dw, dh, dw != ow || dh != oh};
}
// The candidates of each look-ahead list beyond the frame itself, for a handle of this lag and warp mode.  blend_on: the fill's blend rule
// runs; want_sums: the frames' channel sums are measured and travel with the fill's candidates.
struct PassPlan { int fill, deblur, denoise, deflicker, rolling; bool blend_on, want_sums; };
inline PassPlan plan_passes(const PassConfig& c, int lag, int warp_mode) {
    PassPlan p{};
    p.fill = warp_mode == VS_WARP_BILINEAR_CV ? std::min(c.border_fill, lag) : 0;
    p.deblur = std::min(c.deblur, lag);
    p.denoise = std::min(c.denoise, lag);
    p.deflicker = std::min(c.deflicker, lag);
    p.rolling = c.rolling.readout != 0.0 ? std::min(1, lag) : 0;   // the motion to the frame that follows (that frame's pixels are not read)
    p.blend_on = p.fill > 0 && (c.fill_blend.feather > 0 || c.fill_blend.match != 0);
    p.want_sums = p.fill > 0 && c.fill_blend.match != 0;
    return p;
}

// ---- scratch groups and warp runs ---------------------------------------------------------------------------
// Frames per group of a run of run_len frames whose scratch takes per_frame_bytes each and stays within budget; one frame always goes.
inline size_t scratch_group(size_t run_len, size_t budget, size_t per_frame_bytes) {
    return std::min(run_len, std::max<size_t>(1, budget / per_frame_bytes));
}
struct Job { const void* src; vs_transform sampling; int i; void* release; };   // frame i of the chunk is due: warp `src`, then `release` is free
// The end of the run that starts at job j: consecutive frames of the chunk whose sources lie one behind the other -- one warp launch.
inline size_t run_end(const std::vector<Job>& jobs, size_t j, size_t frame_bytes) {
    size_t e = j + 1;
    while (e < jobs.size() && (const uint8_t*)jobs[e].src == (const uint8_t*)jobs[e - 1].src + frame_bytes && jobs[e].i == jobs[e - 1].i + 1) e++;
    return e;
}

}  // namespace stab
}  // namespace vsi
