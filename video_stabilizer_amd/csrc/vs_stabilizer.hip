// vs_stabilizer.hip -- VideoStabilizer (stabilizer.cpp:3-117) on top of the aligner (vs_engine.hip): scalar bookkeeping on the host, frames stay in
// HBM.  Host code only: every kernel it needs is launched by the files it calls (vs_kernels, vs_warp, vs_fill, vs_inpaint, vs_deblur, vs_denoise, vs_rolling, vs_remap, vs_deflicker, vs_scene, vs_sharpen).
//
// Design (DESIGN.md "Engine"): a process call of n frames is one batched alignment, the reference's bookkeeping frame by frame (vs_stab_step.hpp),
// then batched warps of every frame that became due -- stab_chunk, a sequence of named steps.  Around it stab_run picks how a call is cut: host
// batches longer than one upload chunk run as an upload / compute / download pipeline (stab_run_host_pipelined), dense device-resident batches in
// sub-batches whose warps run under the next sub-batch's alignment (stab_run_overlapped).
#include "vs_engine.hpp"
#include "vs_lookahead.hpp"
#include "vs_stab_plan.hpp"
#include "vs_stab_step.hpp"
#include "vs_kernels.hpp"
#include "vs_lens.hpp"
#include "vs_resize.hpp"

#include <algorithm>
#include <array>
#include <deque>
#include <numeric>
#include <string>
#include <vector>

using vsi::set_error;
using vsi::run_async;
using vsi::grow;
using vsi::Scratch;
using namespace vsi::stab;

struct vs_stabilizer {
    vs_stabilizer_params params;
    vs_aligner* aligner = nullptr;
    vs_smoother* smoother = nullptr;
    int frame_index = 0;
    std::deque<vs_transform> measurements;
    std::deque<int> meas_ok;       // the success flag of every entry of `measurements` (border fill: a failed alignment ends a candidate list)
    PassConfig cfg;                // what the vs_stabilizer_set_* calls set (vs_stab_plan.hpp)
    // Fill blend with match on: the three channel sums of every queued frame lie in device memory like the sharpness below: in blocks of the
    // same pool, under the same reference protocol (Held::mb / sums).
    // deblur (vs_deblur.hip): the sharpness of every queued frame lies in device memory, one value per frame in a block taken per call; a block is
    // free again when no queued frame and no launch in flight refers to it (refs; sharp_pending: references given up, counted down at the next point
    // where every reader has been ordered before whatever may refill the block)
    struct SharpBlock { unsigned long long* dev; size_t cap; int refs; };
    std::vector<SharpBlock*> sharp_blocks, sharp_pending;
    // The scratch of the passes, each grown on demand (Scratch::grow) and freed by vs_stabilizer_destroy (scratch()).
    Scratch deblur_buf, denoise_buf, rolling_buf;   // the deblurred / denoised / rolling-shutter-corrected frames of the current call: the source of its warps
    Scratch lens_map;              // lens-distortion correction (vs_remap.hip), in front of everything: the map, made once per (params, w, h) on the device
    bool lens_map_made = false;
    Scratch flicker_buf;           // deflicker: the pair statistics and, behind them, the gains of the current call's output frames
    Scratch inpaint_buf;           // one group of frames: their open counts, their coverage indices, their pyramids
    Scratch sharpen_buf;           // one group of output windows as the warp (fill, inpaint) leaves them: the sharpen's source
    Scratch resize_buf;            // output size set: one group of output windows as the passes leave them, the resize's source
    Scratch scene_prev;            // scene cuts, lag == 0: nothing is queued, so the last frame of a call waits here for the next call's first pair
    bool scene_prev_valid = false;
    Scratch batch_in;              // dense device copy of the current batch (lens correction on: the chunk's frames land there corrected)
    // host callers: cropped outputs of the current chunk on their way down.  Two areas, used alternately by the chunks of a
    // pipelined batch; a downloader thread drains area k on down_stream while the next chunk is computed into area k^1.
    Scratch batch_out[2];
    // PITCHED host frames travel as ONE linear copy of their whole span (gaps included) into a device area and are made dense by device-to-device
    // 2-D copies: the HIP runtime never gets a 2-D copy out of pageable caller memory (profiles/r06_flake.md); dense frames: one linear copy as ever
    Scratch span_in[2];
    std::array<Scratch*, 14> scratch() {
        return {&deblur_buf, &denoise_buf, &rolling_buf, &lens_map, &flicker_buf, &inpaint_buf, &sharpen_buf, &resize_buf, &scene_prev, &batch_in, &batch_out[0],
                &batch_out[1], &span_in[0], &span_in[1]};
    }
    std::deque<int> meas_cut;      // the cut flag of every entry of `measurements` (vs_stab_step.hpp: stab_step_cut); all zero while detection is off
    hipStream_t scene_stream = nullptr;   // overlapped runs: the statistics and their download go beside the next chunk's alignment, which is already
    hipEvent_t scene_ev = nullptr;        // enqueued on the handle's stream; scene_ev: everything on that stream in front of it
    long long cut_total = 0;       // cuts since the last reset
    std::deque<int64_t> cut_list;  // ... the most recent 256 of them: 0-based frame indices since that reset
    struct Held { void* ptr; bool owned; SharpBlock* sb = nullptr; const unsigned long long* sharp = nullptr;
                  SharpBlock* mb = nullptr; const unsigned long long* sums = nullptr; };   // owned: a buffer of ours; else a frame of the batch being processed
    std::deque<Held> frames;       // the buffered input frames (stabilizer.cpp:15), dense, in device memory
    std::vector<void*> pool;       // recycled frame buffers
    size_t frame_bytes = 0;
    std::future<hipError_t> down[2];
    hipEvent_t down_ev[2] = {nullptr, nullptr};
    hipStream_t down_stream = nullptr, up_stream = nullptr;
    void* pipe_in[2] = {nullptr, nullptr}; size_t pipe_in_bytes = 0;     // upload areas of a pipelined host batch (two halves, one size: vsi::grow)
    // device-resident batches: the warps of sub-batch g run on warp_stream under the alignment of sub-batch g + 1 (stab_run_overlapped)
    hipStream_t warp_stream = nullptr;
    hipEvent_t warp_ev = nullptr;
    bool overlap_warps = false;    // set by stab_run_overlapped around its sub-batches
    bool defer_own = false;        // set for all but the last time chunk of one long device-resident clip: frames still queued stay
                                   // pointers into the caller's batch (it outlives the call), only the last chunk copies them out
    std::vector<void*> held_release;   // buffers whose last reader is a warp on warp_stream: back into the pool after its synchronisation
    // alignment results of the chunk being processed [tb] and of the chunk whose alignment is already running [tb ^ 1]
    std::vector<vs_transform> t_buf[2];
    std::vector<int32_t> st_buf[2];
    int tb = 0;
    bool prefetched = false;       // the alignment of the next stab_run_impl call's frames has been started by the previous call
    const void* next_frames = nullptr; int next_n = 0;   // set by stab_run_overlapped: the chunk after the one being processed (0: none)
    vs_transform accum{0, 0, 0, 0}, last_meas{0, 0, 0, 0};
    int last_success = 0;
    int w = 0, h = 0, fmt = -1;
    vsi::YcbcrHold ycbcr;          // vs_stabilizer_process_batch_ycbcr's two BGR buffers (vs_capi_ycbcr.hip); empty unless that entry point is called
};

static void sharp_unhold(vs_stabilizer* s, vs_stabilizer::Held& f) {
    if (f.sb) s->sharp_pending.push_back(f.sb);
    if (f.mb) s->sharp_pending.push_back(f.mb);
    f.sb = nullptr; f.sharp = nullptr;
    f.mb = nullptr; f.sums = nullptr;
}
static void sharp_settle(vs_stabilizer* s) {
    for (auto* b : s->sharp_pending) --b->refs;
    s->sharp_pending.clear();
}
static void stab_drop_frames(vs_stabilizer* s) {
    for (auto& f : s->frames) { sharp_unhold(s, f); if (f.owned) (void)hipFree(f.ptr); }
    for (void* p : s->pool) (void)hipFree(p);
    s->frames.clear();
    s->pool.clear();
}

extern "C" {

vs_stabilizer* vs_stabilizer_create(const vs_stabilizer_params* params, int device) try {
    vs_stabilizer_params p;
    if (params) p = *params; else vs_stabilizer_params_default(&p);
    vs_aligner* a = vs_aligner_create(&p.aligner, device);
    if (!a) return nullptr;
    // the aligner owns streams and device slabs: whatever fails from here on releases it (a host allocation that throws included)
    struct Guard { vs_aligner* a; ~Guard() { if (a) vs_aligner_destroy(a); } } guard{a};
    vs_stabilizer* s = new vs_stabilizer();
    s->params = p;
    s->aligner = a;
    guard.a = nullptr;                                     // (from here vs_stabilizer_destroy releases it)
    s->smoother = vs_smoother_create(p.lag, p.smoother_memory, p.lambda);   // stabilizer.cpp:4
    if (!s->smoother) { vs_stabilizer_destroy(s); return nullptr; }         // (last error: the smoother's)
    return s;
} VS_CATCH_ALL_NULL

void vs_stabilizer_destroy(vs_stabilizer* s) {
    if (!s) return;
    (void)hipSetDevice(vsi::aligner_device(s->aligner));
    stab_drop_frames(s);
    for (auto& f : s->down) if (f.valid()) (void)f.get();
    for (auto* b : s->sharp_blocks) { (void)hipFree(b->dev); delete b; }
    for (Scratch* b : s->scratch()) b->drop();
    if (s->scene_stream) { (void)vsi::retire_stream(s->scene_stream); (void)hipStreamDestroy(s->scene_stream); }
    if (s->scene_ev) (void)hipEventDestroy(s->scene_ev);
    for (void* q : s->ycbcr.buf) if (q) (void)hipFree(q);
    for (void* q : s->pipe_in) if (q) (void)hipFree(q);
    for (hipEvent_t e : s->down_ev) if (e) (void)hipEventDestroy(e);
    if (s->warp_stream) { (void)vsi::retire_stream(s->warp_stream); (void)hipStreamDestroy(s->warp_stream); }
    if (s->warp_ev) (void)hipEventDestroy(s->warp_ev);
    if (s->down_stream) (void)hipStreamDestroy(s->down_stream);
    if (s->up_stream) (void)hipStreamDestroy(s->up_stream);
    vs_smoother_destroy(s->smoother);
    vs_aligner_destroy(s->aligner);
    delete s;
}

}  // extern "C"

namespace vsi {
YcbcrHold* stab_ycbcr_hold(vs_stabilizer* s) { return &s->ycbcr; }
int stab_crop(const vs_stabilizer* s) { return s->params.crop_pixels > 0 ? s->params.crop_pixels : 0; }
int stab_device(const vs_stabilizer* s) { return aligner_device(s->aligner); }
void stab_delivered_size(const vs_stabilizer* s, int w, int h, int* dw, int* dh) {
    const Delivery d = delivered_size(w, h, stab_crop(s), s->cfg);
    *dw = d.w; *dh = d.h;
}
}  // namespace vsi

// One vs_stabilizer_process_batch / _clips call, or a run of its frames; strides in elements.  clip_len > 0: the n frames are n / clip_len
// independent clips, each run through a fresh stabilizer (reset before every clip and after the last), all of them aligned and warped together.
struct StabCall {
    const void* frames; size_t frame_stride; int n, clip_len, w, h, stride, format, mem;
    void* out; size_t out_frame_stride; int32_t* has_output; int* out_w; int* out_h;

    size_t esz() const { return vs_format_bits(format) > 8 ? 2 : 1; }
    size_t fbytes() const { return (size_t)w * h * 3 * esz(); }              // one dense frame
    size_t span_bytes() const { return ((size_t)(n - 1) * frame_stride + (size_t)(h - 1) * stride + (size_t)3 * w) * esz(); }   // first to last sample
    bool dense() const { return stride == 3 * w && (n == 1 || frame_stride == (size_t)h * stride); }
    const uint8_t* frame(int i) const { return (const uint8_t*)frames + (size_t)i * frame_stride * esz(); }
    uint8_t* out_frame(int i) const { return (uint8_t*)out + (size_t)i * out_frame_stride * esz(); }
    // the call for frames f0 .. f0 + m; the same call with its frames dense in device memory at `p`
    StabCall sub(int f0, int m) const { StabCall c = *this; c.frames = frame(f0); c.out = out_frame(f0); c.has_output = has_output + f0; c.n = m; return c; }
    StabCall dense_at(const void* p) const { StabCall c = *this; c.frames = p; c.frame_stride = (size_t)w * h * 3; c.stride = 3 * w; c.mem = VS_MEM_DEVICE; return c; }
};

// The frames of `c` (host or device memory, any pitch) dense at `dst` in device memory, on `st`.  dense: they lie dense where they are -- one
// linear copy at the full link rate.  Pitched host frames go through span_in[area] (see there); pitched device frames are 2-D copies.
static hipError_t make_dense(vs_stabilizer* s, const StabCall& c, bool dense, int area, void* dst, hipStream_t st) {
    const size_t esz = c.esz(), fbytes = c.fbytes(), row = (size_t)c.w * 3 * esz;
    if (dense) return hipMemcpyAsync(dst, c.frames, fbytes * c.n, c.mem == VS_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st);
    const uint8_t* from = (const uint8_t*)c.frames;
    hipError_t e = hipSuccess;
    if (c.mem == VS_MEM_HOST) {
        const size_t span = c.span_bytes();
        e = s->span_in[area].grow(span);
        if (e == hipSuccess) e = hipMemcpyAsync(s->span_in[area].p, c.frames, span, hipMemcpyHostToDevice, st);
        from = (const uint8_t*)s->span_in[area].p;
    }
    for (int i = 0; e == hipSuccess && i < c.n; i++)
        e = hipMemcpy2DAsync((uint8_t*)dst + (size_t)i * fbytes, row, from + (size_t)i * c.frame_stride * esz, (size_t)c.stride * esz, row, c.h,
                             hipMemcpyDeviceToDevice, st);
    return e;
}

// The outputs of input frames idx[0], idx[1], .. lie dense in `area`, obytes (a delivered frame) each; down to the caller's frames on `st`, runs that are contiguous on
// both sides as one copy.
static hipError_t copy_outputs_down(const StabCall& c, const std::vector<int>& idx, const uint8_t* area, size_t obytes, hipStream_t st) {
    const bool dense_out = c.out_frame_stride * c.esz() == obytes;
    hipError_t e = hipSuccess;
    for (size_t j = 0; e == hipSuccess && j < idx.size();) {
        size_t k = j + 1;
        while (dense_out && k < idx.size() && idx[k] == idx[k - 1] + 1) k++;
        e = hipMemcpyAsync(c.out_frame(idx[j]), area + j * obytes, obytes * (k - j), hipMemcpyDeviceToHost, st);
        j = k;
    }
    return e;
}

// ---- one chunk: n successive VideoStabilizer::processFrame calls (stabilizer.cpp:9-117) as one batch ---------------------------------------
using Held = vs_stabilizer::Held;
using SharpBlock = vs_stabilizer::SharpBlock;
// The look-ahead passes (DESIGN.md "Look-ahead passes: the shared path"): per job 1 + n candidates -- the frame itself, then the frames
// that follow it in the queue; null frames and zero transforms behind the end of a list.  `side`: where each candidate's side value lies.
struct Ahead { int n; std::vector<const void*> src; std::vector<vs_transform> t; std::vector<const uint64_t*> side; };

// an idle block of at least `need` values, or a new one (`keep`: a block taken earlier in this call, still without references)
static int take_block(vs_stabilizer* s, size_t need, SharpBlock* keep, SharpBlock** out) {
    for (auto* b : s->sharp_blocks) if (b != keep && b->refs == 0 && b->cap >= need) { *out = b; return VS_OK; }
    for (auto it = s->sharp_blocks.begin(); it != s->sharp_blocks.end();)           // idle blocks that are too small make room
        if (*it != keep && (*it)->refs == 0) { (void)hipFree((*it)->dev); delete *it; it = s->sharp_blocks.erase(it); } else ++it;
    void* q = nullptr;
    VS_HIP(vsi::dev_alloc(&q, need * sizeof(unsigned long long)));
    s->sharp_blocks.reserve(s->sharp_blocks.size() + 1);
    *out = new SharpBlock{(unsigned long long*)q, need, 0};
    s->sharp_blocks.push_back(*out);
    return VS_OK;
}

// The byte budget of a pass's scratch groups (vs_stab_plan.hpp: scratch_group).  (hook_name: a test hook, read at every call, in place of the
// budget, so that clips of a few frames run in several groups)
static size_t scratch_budget(const char* hook_name, size_t default_bytes) {
    const char* const hook = vsi::test_env(hook_name);
    return hook ? (size_t)strtoull(hook, nullptr, 0) : default_bytes;
}

// One chunk in flight: what its steps share, and the steps in the order stab_chunk runs them.
struct Chunk {
    vs_stabilizer* s;
    const StabCall& c;
    int slot;                      // the output area (batch_out / down) that host outputs leave through
    bool threaded_download;        // ... with a downloader thread of their own, under the next chunk's compute
    bool to_host, warps_apart;     // the outputs go to host memory (a chunk of the pipelined host batch too); the warps go to warp_stream
    hipStream_t st, ws;            // the handle's stream; the stream of the passes and the warps
    int crop, ow, oh;              // the crop window: what the warp, the fill, the inpaint, the sharpen and the deflicker's gain work on
    int dw, dh; bool resize_on;    // the delivered frame (vs_stab_plan.hpp: delivered_size): the window, or the window resized behind everything
    int w = c.w, h = c.h, fbits = vs_format_bits(c.format), bits = fbits > 8 ? 16 : 8;
    size_t fbytes = c.fbytes(), obytes = (size_t)ow * oh * 3 * c.esz(), dbytes = (size_t)dw * dh * 3 * c.esz();
    const uint8_t* dense = nullptr; bool already_dense = false;   // the chunk's frames, dense, in device memory; ... where the caller has them
    SharpBlock *sblk = nullptr, *mblk = nullptr;   // the sharpness of the chunk's frames (deblur on); their channel sums (fill with exposure match)
    bool blend_on = false, want_sums = false;
    int cur = 0;                   // t_buf[cur] / st_buf[cur]: the chunk's alignment results
    std::vector<Job> jobs;
    Ahead fill{}, db{}, dn{}, fk{};    // border fill (side, exposure match only: the channel sums, the ORIGINAL frames' throughout); deblur (side: the
                                       // sharpness); denoise; deflicker (candidate 0 stays the ORIGINAL frame whatever deblur and denoise do)
    Ahead rs{};                        // rolling shutter: depth min(1, lag) -- the motion to the frame that follows (that frame's pixels are not read)
    uint32_t* fk_gains = nullptr;  // deflicker: four words per job, in flicker_buf
    std::vector<uint8_t> cuts;     // scene-cut detection: frame i of the chunk shows another scene than its predecessor (all zero while it is off)
    hipStream_t cut_stream = st;   // ... where its statistics run: scene_stream once the next chunk's alignment has been enqueued on `st`

    // stabilizer.cpp:15: a private dense copy of every input frame, in device memory
    // With the lens correction on the frames land there corrected: the remap reads device frames in place, whatever their pitch, and host frames
    // from span_in[0], where their whole span travels as one linear copy; the aligner, the side values, the queue and every pass then see
    // corrected frames only.  (already_dense stays false: no next chunk's alignment is started on the caller's uncorrected frames.)
    int make_dense() {
        if (s->cfg.lens_on) return make_dense_corrected();
        already_dense = c.mem == VS_MEM_DEVICE && c.dense();
        dense = (const uint8_t*)c.frames;                  // read in place during this call; the tail is copied out by own_queued
        if (already_dense) return VS_OK;
        VS_HIP(s->batch_in.grow(fbytes * c.n));
        VS_HIP(::make_dense(s, c, c.dense(), 0, s->batch_in.p, st));
        dense = (const uint8_t*)s->batch_in.p;
        return VS_OK;
    }

    int make_dense_corrected() {
        if (!s->lens_map_made) {                           // once per (params, w, h): vs_stabilizer_set_lens drops it
            VS_HIP(s->lens_map.grow((size_t)w * h * 2 * sizeof(int32_t)));
            VS_HIP(vsk::lens_map(s->cfg.lens, w, h, (int32_t*)s->lens_map.p, 2 * w, st));
            s->lens_map_made = true;
        }
        const void* from = c.frames;
        if (c.mem == VS_MEM_HOST) {
            VS_HIP(s->span_in[0].grow(c.span_bytes()));
            VS_HIP(hipMemcpyAsync(s->span_in[0].p, c.frames, c.span_bytes(), hipMemcpyHostToDevice, st));
            from = s->span_in[0].p;
        }
        VS_HIP(s->batch_in.grow(fbytes * c.n));
        VS_HIP(vsk::bgr_remap(from, c.frame_stride, c.n, w, h, c.stride, bits, vs_format_max_value(c.format), (const int32_t*)s->lens_map.p, 2 * w, w, h,
                              s->cfg.lens.border, s->batch_in.p, (size_t)w * h * 3, w * 3, vsk::kRemapSlice, st));
        dense = (const uint8_t*)s->batch_in.p;
        return VS_OK;
    }

    // `per` values per frame, measured by launch(frames, where to, how many, frame stride): the call's n frames in one launch into a block of
    // their own (*out), then every queued frame that lacks the value, one launch each, behind them in the same block
    template <typename Launch>
    int measure(size_t per, SharpBlock* keep, SharpBlock* Held::*blk, const unsigned long long* Held::*val, Launch launch, SharpBlock** out) {
        size_t need = (size_t)c.n;
        for (auto& f : s->frames) if (!(f.*blk)) need++;
        VS_TRY(take_block(s, per * need, keep, out));
        VS_HIP(launch(dense, (*out)->dev, c.n, (size_t)w * h * 3));
        size_t at = (size_t)c.n;
        for (auto& f : s->frames) {
            if (f.*blk) continue;
            VS_HIP(launch(f.ptr, (*out)->dev + per * at, 1, 0));
            f.*blk = *out; f.*val = (*out)->dev + per * at; ++(*out)->refs; at++;
        }
        return VS_OK;
    }
    // The side values of the chunk's frames, one launch over all of them each, into a block of their own; the values stay on the device.
    int measure_side_values() {
        if (!s->overlap_warps) sharp_settle(s);
        // deblur (vs_deblur.hip): the sharpness.  (Queued frames that arrived while deblur was off are measured here too, once.)
        if (db.n > 0)
            VS_TRY(measure(1, nullptr, &Held::sb, &Held::sharp, [&](const void* p, unsigned long long* to, int m, size_t fs) {
                return vsk::bgr_sharpness(p, w, h, w * 3, bits, fbits - 8, to, m, fs, st); }, &sblk));
        // fill blend with exposure match (vs_fill.hip): the three channel sums.  (Queued frames that arrived while the match was off are summed
        // here too, once: switching on mid-clip gives what a handle that had it from the first frame gives.)
        if (want_sums)
            VS_TRY(measure(3, sblk, &Held::mb, &Held::sums, [&](const void* p, unsigned long long* to, int m, size_t fs) {
                return vsk::bgr_channel_sums(p, w, h, w * 3, bits, to, m, fs, st); }, &mblk));
        if ((db.n > 0 || want_sums) && warps_apart) {       // the deblur pass / the fill's gain kernel read the values on warp_stream
            VS_HIP(hipEventRecord(s->warp_ev, st));
            VS_HIP(hipStreamWaitEvent(s->warp_stream, s->warp_ev, 0));
        }
        return VS_OK;
    }

    // stabilizer.cpp:18-19 for all n frames.  In a chunked device-resident batch (stab_run_overlapped) the alignment of the NEXT chunk is
    // started as soon as this one's results are in, so that it runs under this chunk's host work (smoother, correction chain, warp
    // launches) as well as under its warps.
    int align() {
        vs_aligner* a = s->aligner;
        cur = s->tb;
        auto start = [&](int into, const void* frames, int n, bool async) {
            s->t_buf[into].resize(n);
            s->st_buf[into].resize(n);
            return vsi::align_start(a, frames, (size_t)w * h * 3, n, c.clip_len, w, h, w * 3, c.format, VS_MEM_DEVICE, &s->params.aligner,
                                    s->t_buf[into].data(), s->st_buf[into].data(), async);
        };
        if (s->prefetched) s->prefetched = false;           // started by the previous call, into [cur]
        else VS_TRY(start(cur, dense, c.n, false));
        VS_TRY(vsi::align_finish(a));
        if (s->next_n > 0 && already_dense) {
            if (s->cfg.scene_on) {                              // detect_cuts works beside the alignment started here, behind what `st` holds now
                if (!s->scene_stream) VS_HIP(hipStreamCreateWithFlags(&s->scene_stream, hipStreamNonBlocking));
                if (!s->scene_ev) VS_HIP(hipEventCreateWithFlags(&s->scene_ev, hipEventDisableTiming));
                VS_HIP(hipEventRecord(s->scene_ev, st));
                VS_HIP(hipStreamWaitEvent(s->scene_stream, s->scene_ev, 0));
                cut_stream = s->scene_stream;
            }
            VS_TRY(start(cur ^ 1, s->next_frames, s->next_n, true));
            s->prefetched = true;
            s->tb = cur ^ 1;
        }
        return VS_OK;
    }

    // Scene-cut detection (vs_scene.hip): every frame of the call that has a predecessor in the same clip is compared with
    // it through the motion just measured -- the pair (frame j-1, frame j, t), t from lookahead_transforms over the single measurement T_j, so
    // that its direction is the look-ahead passes' by construction.  One statistics launch, one download of two words per pair through the
    // pinned staging of the kernel-level calls, the decision on the host.  The predecessor of the call's first frame is the back of the queue
    // (lag == 0: the handle's copy of the previous call's last frame).  Off: nothing is launched and nothing allocated.
    int detect_cuts() {
        cuts.assign((size_t)c.n, 0);
        if (!s->cfg.scene_on) return VS_OK;
        std::vector<const void*> src;
        std::vector<vs_transform> t;
        std::vector<int> at;
        const int one = 1;
        for (int i = 0; i < c.n; i++) {
            const void* prev = nullptr;
            if (c.clip_len > 0 ? i % c.clip_len != 0 : i > 0) prev = dense + (size_t)(i - 1) * fbytes;
            else if (c.clip_len > 0) continue;              // a clip's first frame
            else if (!s->frames.empty()) prev = s->frames.back().ptr;
            else if (s->scene_prev_valid) prev = s->scene_prev.p;
            if (!prev) continue;
            vs_transform tr;
            (void)vsi::lookahead_transforms(&s->t_buf[cur][i], &one, 1, 1, nullptr, &tr);
            src.push_back(prev);
            src.push_back(dense + (size_t)i * fbytes);
            t.push_back(tr);
            at.push_back(i);
        }
        if (at.empty()) return VS_OK;
        const int np = (int)at.size();
        std::vector<uint64_t> stats(2 * (size_t)np);
        {
            vsi::Staged o;
            VS_TRY(o.out(stats.data(), stats.size() * sizeof(uint64_t), VS_MEM_HOST));
            VS_TRY(vsi::scene_stats_ptrs(np, w, h, w * 3, c.format, src.data(), t.data(), &s->cfg.scene_params, o.as<uint64_t>(), cut_stream));
            VS_TRY(vsi::finish_outputs(VS_MEM_HOST, cut_stream, {&o}));
        }
        std::vector<uint8_t> flag((size_t)np);
        VS_TRY(vs_scene_cuts(stats.data(), np, w, h, &s->cfg.scene_params, flag.data()));
        for (int k = 0; k < np; k++) cuts[(size_t)at[k]] = flag[(size_t)k];
        return VS_OK;
    }
    // lag == 0: the call's last frame waits in a buffer of the handle's for the next call's first pair
    int keep_last_frame() {
        if (!s->cfg.scene_on || s->params.lag > 0 || c.clip_len > 0) return VS_OK;
        VS_HIP(s->scene_prev.grow(fbytes));   // (its one reader, detect_cuts, has synchronised)
        VS_HIP(hipMemcpyAsync(s->scene_prev.p, dense + (size_t)(c.n - 1) * fbytes, fbytes, hipMemcpyDeviceToDevice, st));
        s->scene_prev_valid = true;
        return VS_OK;
    }

    // Frame `src` has left the queue, due under `correction`: its candidate lists.  The queue now holds the frames k+1 .. behind this frame k,
    // `measurements` their motions T_{k+1} .. (T_j: frame j-1 to j), entry for entry.  Frame j shows frame k's pixels through
    // inverse(T_{k+1} o .. o T_j), and -- the fill -- this output through F_j = compose(that, correction); a frame whose alignment failed ends
    // the list (vs_lookahead.hpp).  (The frames are read before their own jobs release them: releases follow all launches.)
    void lists(const Held& src, const vs_transform& correction) {
        const size_t avail = std::min(s->frames.size(), s->measurements.size());
        auto list = [&](Ahead& a, size_t have, const vs_transform& t0, const vs_transform* corr, const unsigned long long* Held::*side) {
            if (a.n <= 0) return;
            a.src.push_back(src.ptr);
            a.t.push_back(t0);
            const size_t at = a.t.size();
            a.t.resize(at + (size_t)a.n);
            const int live = vsi::lookahead_transforms(s->measurements, s->meas_ok, have, a.n, corr, &a.t[at]);
            for (int i = 0; i < a.n; i++) a.src.push_back(i < live ? s->frames[i].ptr : nullptr);
            if (!side) return;
            a.side.push_back((const uint64_t*)(src.*side));
            for (int i = 0; i < a.n; i++) a.side.push_back(i < live ? (const uint64_t*)(s->frames[i].*side) : nullptr);
        };
        const vs_transform none{0, 0, 0, 0};
        list(fill, avail, correction, &correction, want_sums ? &Held::sums : nullptr);
        size_t sharp_avail = 0;                     // the deblur's list also ends at a frame without a sharpness value
        while (sharp_avail < avail && s->frames[sharp_avail].sharp) sharp_avail++;
        list(db, sharp_avail, none, nullptr, &Held::sharp);
        list(dn, avail, none, nullptr, nullptr);
        list(fk, avail, none, nullptr, nullptr);
        list(rs, avail, none, nullptr, nullptr);
    }
    // The frame loop: every frame joins the queue, its measurement goes through the reference's bookkeeping (vs_stab_step.hpp), and the frame
    // that becomes due leaves the queue as a job with its candidate lists.
    int frame_loop() {
        for (int i = 0; i < c.n; i++) {
            if (c.clip_len > 0 && i % c.clip_len == 0) VS_TRY(vs_stabilizer_reset(s));   // a new clip: frames still queued are dropped
            ++s->frame_index;
            s->frames.push_back(Held{(void*)(dense + (size_t)i * fbytes), false, sblk, sblk ? sblk->dev + i : nullptr, mblk,
                                     mblk ? mblk->dev + 3 * (size_t)i : nullptr});
            if (sblk) ++sblk->refs;
            if (mblk) ++mblk->refs;
            const bool cut = cuts[(size_t)i] != 0;
            const vs_transform meas = cut ? vs_transform{0, 0, 0, 0} : s->t_buf[cur][i];
            const bool success = s->st_buf[cur][i] == 1;
            s->last_meas = meas; s->last_success = success && !cut ? 1 : 0;
            if (cut) {
                ++s->cut_total;
                if (s->cut_list.size() == 256) s->cut_list.pop_front();
                s->cut_list.push_back((int64_t)s->frame_index - 1);
            }
            c.has_output[i] = 0;
            vs_transform correction;
            if (!vsi::stab_step_cut(meas, success, cut, w, h, s->params, s->smoother, s->measurements, s->meas_ok, s->meas_cut, s->accum, &correction)) continue;
            if (s->frames.empty()) continue;
            const Held src = s->frames.front();
            s->frames.pop_front();
            if (src.sb) s->sharp_pending.push_back(src.sb);   // (the jobs' launches still read it: counted down after them)
            if (src.mb) s->sharp_pending.push_back(src.mb);
            // :97-99: warpBySimilarityTransform(frame, accum^-1); cv::warpAffine without WARP_INVERSE_MAP
            // inverts the matrix it is given (imgproc.cpp:472), so the sampling map is (accum^-1)^-1.
            // (VS_WARP_BILINEAR_CV is cv::warpAffine itself, inversion included: it takes the correction as the reference hands it over)
            jobs.push_back(Job{src.ptr, s->params.warp_mode == VS_WARP_BILINEAR_CV ? correction : vs_transform_inverse(&correction), i,
                               src.owned ? src.ptr : nullptr});
            c.has_output[i] = 1;
            lists(src, correction);
        }
        return VS_OK;
    }

    // One pass that rewrites every due frame (`a` on): its scratch grows, candidate 0 of every list is the job's current source (the deblur,
    // first in line, finds it there already), launch(to) writes the frames to the scratch one after the other, and there the warps (and the
    // fill's candidate 0) read them from now on.
    template <typename Launch>
    int rewrite(Ahead& a, Scratch& buf, Launch launch) {
        if (a.n <= 0) return VS_OK;
        VS_HIP(buf.grow(fbytes * jobs.size(), ws, true));
        for (size_t j = 0; j < jobs.size(); j++) a.src[j * (1 + a.n)] = jobs[j].src;
        VS_TRY(launch(buf.p));
        for (size_t j = 0; j < jobs.size(); j++) {
            jobs[j].src = (const uint8_t*)buf.p + j * fbytes;
            if (fill.n > 0) fill.src[j * (1 + fill.n)] = jobs[j].src;
        }
        return VS_OK;
    }
    // The look-ahead passes that run in front of the warps, on their stream, one launch each over every due frame.  The candidates are read
    // before their own jobs release them: releases follow the warps.  (sync in grow: warps / gain passes of an earlier chunk may still read the
    // area.)  Host callers first: the staging area's previous user has been drained (through down[slot]), and the area holds the jobs' outputs.
    int passes() {
        const int nj = (int)jobs.size();
        if (to_host) {
            if (s->down[slot].valid()) {
                const hipError_t de = s->down[slot].get();
                if (de != hipSuccess) return set_error(VS_ERR_HIP, "output download failed: %s", hipGetErrorString(de));
            }
            VS_HIP(s->batch_out[slot].grow(dbytes * jobs.size()));
        }
        const size_t fs = (size_t)w * h * 3;
        // every due frame is deblurred into a scratch frame of its own
        VS_TRY(rewrite(db, s->deblur_buf, [&](void* to) {
            return vsi::bgr_deblur_ptrs(nj, w, h, w * 3, c.format, 1 + db.n, db.src.data(), db.side.data(), db.t.data(), &s->cfg.deblur_params, to, fs, w * 3, ws); }));
        // ... (deblurred, if that pass is on) denoised into a scratch frame of its own; the candidates are the original input frames
        VS_TRY(rewrite(dn, s->denoise_buf, [&](void* to) {
            return vsi::bgr_denoise_ptrs(nj, w, h, w * 3, c.format, 1 + dn.n, dn.src.data(), dn.t.data(), &s->cfg.denoise_params, to, fs, w * 3, ws); }));
        // ... (deblurred, denoised) corrected for the rolling shutter into a scratch frame of its own, by the motion to the next input frame
        VS_TRY(rewrite(rs, s->rolling_buf, [&](void* to) {
            return vsi::bgr_rolling_ptrs(nj, w, h, w * 3, c.format, rs.src.data(), rs.t.data(), &s->cfg.rolling, to, fs, w * 3, ws); }));
        if (fk.n > 0) {
            // the exposure statistics of every due frame against the frames that follow it -- the original input frames on both sides -- and
            // its three gains: one statistics launch and one gains launch.  Nothing of it reaches the host; the gain pass behind each run's
            // warp (and fill) reads the gains there.
            const size_t sbytes = jobs.size() * (size_t)(1 + fk.n) * 8 * sizeof(uint64_t), need = sbytes + jobs.size() * 4 * sizeof(uint32_t);
            VS_HIP(s->flicker_buf.grow(need, ws, true));
            fk_gains = (uint32_t*)((uint8_t*)s->flicker_buf.p + sbytes);
            VS_TRY(vsi::exposure_stats_ptrs(nj, w, h, w * 3, c.format, 1 + fk.n, fk.src.data(), fk.t.data(), &s->cfg.deflicker_params,
                                            (uint64_t*)s->flicker_buf.p, ws));
            VS_HIP(vsk::exposure_gains((const unsigned long long*)s->flicker_buf.p, nj, 1 + fk.n, w, h, s->cfg.deflicker_params.step, fk_gains, ws));
        }
        return VS_OK;
    }

    // Inpaint of frames [j, e) of the jobs, whose output windows lie at `dst`: the coverage index from the run's fill list (fill off: candidate 0
    // alone), then the push-pull in place.  A run whose frames all cover their window themselves launches nothing: the same int32 rectangle
    // test as the kernels', on the host (vs_lookahead.hpp), so the default crop pays a handful of host operations per frame.  The frames go
    // in groups whose scratch -- open counts, coverage indices (rows padded to dwords), pyramids -- stays within kInpaintScratch.  256 MB:
    // thirteen 4K 8-bit frames (8.3 MB of index + 11 MB of pyramid each) or eight 4K 16-bit ones.  The pass is a chain of some fifteen
    // launches per group whose length is set by latency, not by bytes (the rim blocks' strip walk, the small upper levels, the tail), so a
    // group has to be large to amortise it: with 64 MB -- three frames -- a 4K frame paid 65-116 us instead of 45-56.  The deblur's and the denoise's scratch hold a
    // full frame per due frame of the call; this stays below them.  A single frame that needs more gets what it needs.  Every byte of the
    // scratch that is read has been written in the same group: the count by a memset, the index by the coverage kernel (every window
    // pixel), a pyramid level by the push in front of its readers; idle frames' pyramids are never read.
    static constexpr size_t kInpaintScratch = (size_t)256 << 20;
    int inpaint_run(size_t j, size_t e, void* dst, size_t dst_fs) {
        const int nfill = fill.n, nc = 1 + nfill;
        std::vector<const void*> src1;
        std::vector<vs_transform> t1;
        const void* const* srcs; const vs_transform* tr;
        if (nfill > 0) { srcs = &fill.src[j * nc]; tr = &fill.t[j * nc]; }
        else {
            for (size_t q = j; q < e; q++) { src1.push_back(jobs[q].src); t1.push_back(jobs[q].sampling); }
            srcs = src1.data(); tr = t1.data();
        }
        bool all_covered = true;
        for (size_t q = j; all_covered && q < e; q++) {
            double M[6];
            vs_cv_inverse_matrix(&tr[(q - j) * nc], w, h, M);
            all_covered = vsi::cv_window_covered(M, crop, crop, ow, oh, w, h);
        }
        if (all_covered) return VS_OK;
        const int ms = (ow + 3) & ~3;
        const size_t mfs = (size_t)ms * oh, pbytes = (vsk::inpaint_pyramid_bytes(ow, oh, bits) + 15) & ~(size_t)15;
        const size_t group = scratch_group(e - j, scratch_budget("VS_TEST_INPAINT_SCRATCH_BYTES", kInpaintScratch), mfs + pbytes + sizeof(uint32_t));
        const size_t cbytes = (group * sizeof(uint32_t) + 255) & ~(size_t)255;
        VS_HIP(s->inpaint_buf.grow(cbytes + group * (mfs + pbytes), ws, true));   // (an earlier run's kernels may still read the block)
        uint32_t* const counts = (uint32_t*)s->inpaint_buf.p;
        uint8_t* const cov = (uint8_t*)s->inpaint_buf.p + cbytes;
        void* const pyr = cov + group * mfs;
        for (size_t g = j; g < e; g += group) {
            const int m = (int)std::min(group, e - g);
            VS_TRY(vsi::fill_coverage_ptrs(m, w, h, nc, srcs + (g - j) * nc, tr + (g - j) * nc, crop, crop, ow, oh, cov, mfs, ms, counts, ws, "vs_stabilizer_set_inpaint"));
            VS_HIP(vsk::bgr_inpaint((uint8_t*)dst + (g - j) * dst_fs * c.esz(), dst_fs, m, ow, oh, ow * 3, bits, cov, mfs, ms, counts, pyr, ws));
        }
        return VS_OK;
    }

    // warp every due frame, runs of consecutive batch frames as one launch.  The crop of stabilizer.cpp:102-109 is the
    // output window of the warp: the margin is never computed and no full-size intermediate frame exists.  Device callers
    // get the window written straight into `out`; host callers into the staging area.
    int warp_runs() {
        const int nfill = fill.n, max_value = vs_format_max_value(c.format);
        // (device output of an overlapped clip batch: the warps go to warp_stream and run under the next group's alignment; beside it the
        // Lanczos2 warp keeps its standard window: see vsi::warp_keeps_solver_slot)
        struct SlotHint { bool& f; bool old; SlotHint(bool on) : f(vsi::warp_keeps_solver_slot()), old(f) { f = on; } ~SlotHint() { f = old; } } hint(s->overlap_warps);
        std::vector<vs_transform> ts;
        // Sharpen on: a run goes in groups whose windows, as the warp (fill, inpaint) leaves them, lie dense in the handle's scratch; the sharpen
        // writes them to where the warp wrote them before, each under its own frame's correction.  The scratch holds kSharpenScratch bytes or
        // one window, whichever is more, and no more than the call's due frames need: one allocation for all runs of the call (sync in grow:
        // an earlier call's sharpen may still read the block).  256 MB: forty-three 1080p or ten 4K 8-bit windows -- launches that long are
        // bound by bytes, not by their count.
        size_t max_group = jobs.size();
        if (s->cfg.sharpen_on && !jobs.empty()) {
            max_group = scratch_group(max_group, scratch_budget("VS_TEST_SHARPEN_SCRATCH_BYTES", kSharpenScratch), obytes);
            VS_HIP(s->sharpen_buf.grow(max_group * obytes, ws, true));
        }
        // Output size set: the group's windows, as every pass above leaves them, lie dense in resize_buf, and the resize writes the delivered
        // frames to where the windows went before -- last on the run's stream.  The same grouping rule and budget as the sharpen's scratch.
        if (resize_on && !jobs.empty()) {
            max_group = scratch_group(max_group, scratch_budget("VS_TEST_RESIZE_SCRATCH_BYTES", kResizeScratch), obytes);
            VS_HIP(s->resize_buf.grow(max_group * obytes, ws, true));
        }
        for (size_t j = 0, e; j < jobs.size(); j = e) {
            e = run_end(jobs, j, fbytes);
            ts.clear();
            for (size_t q = j; q < e; q++) ts.push_back(jobs[q].sampling);
            void* dst = to_host ? (void*)((uint8_t*)s->batch_out[slot].p + j * dbytes) : (void*)c.out_frame(jobs[j].i);
            const size_t dst_fs = to_host ? (size_t)dw * dh * 3 : c.out_frame_stride;
            // (sharpen and resize off: one group, the run itself, written where it always went)
            const size_t group = std::min(e - j, max_group);
            for (size_t g = j, ge; g < e; g = ge) {
                ge = std::min(e, g + group);
                const int m = (int)(ge - g);
                void* const delivered = (uint8_t*)dst + (g - j) * dst_fs * c.esz();
                void* const out = resize_on ? s->resize_buf.p : delivered;          // the group's windows
                const size_t out_fs = resize_on ? (size_t)ow * oh * 3 : dst_fs;
                void* const wdst = s->cfg.sharpen_on ? s->sharpen_buf.p : out;
                const size_t wfs = s->cfg.sharpen_on ? (size_t)ow * oh * 3 : out_fs;
                if (nfill > 0)     // the same warp launch, then the fill pass over the uncovered rim on the same stream
                    VS_TRY(vsi::bgr_warp_fill_ptrs(jobs[g].src, (size_t)w * h * 3, m, w, h, w * 3, bits, 1 + nfill, &fill.src[g * (1 + nfill)],
                                                   &fill.t[g * (1 + nfill)], s->params.warp_border, max_value, crop, crop, ow, oh, wdst, wfs, ow * 3, ws,
                                                   want_sums ? &fill.side[g * (1 + nfill)] : nullptr, blend_on ? &s->cfg.fill_blend : nullptr));
                else
                    VS_TRY(vs_bgr_image_warp_roi_batch(jobs[g].src, (size_t)w * h * 3, m, w, h, w * 3, 3, bits, &ts[g - j], s->params.warp_mode,
                                                       s->params.warp_border, max_value, crop, crop, ow, oh, wdst, wfs, ow * 3, VS_MEM_DEVICE, ws));
                if (s->cfg.inpaint) VS_TRY(inpaint_run(g, ge, wdst, wfs));
                if (s->cfg.sharpen_on)
                    VS_TRY(vsi::bgr_sharpen_ptrs(wdst, wfs, m, w, h, c.format, &ts[g - j], &s->cfg.sharpen, crop, crop, ow, oh, ow * 3, out, out_fs, ow * 3, ws));
                // deflicker: the group's output windows scaled in place by their frames' gains, last on the run's stream (in front of any download)
                if (fk.n > 0)
                    VS_HIP(vsk::bgr_gain(out, ow, oh, ow * 3, bits, max_value, fk_gains + 4 * g, out, ow * 3, m, out_fs, out_fs, ws));
                if (resize_on)
                    VS_TRY(vs_bgr_resize_batch(out, out_fs, m, ow, oh, ow * 3, c.format, s->cfg.out_filter, delivered, dst_fs, dw, dh, dw * 3, VS_MEM_DEVICE, ws));
            }
        }
        return VS_OK;
    }
    static constexpr size_t kSharpenScratch = (size_t)256 << 20, kResizeScratch = (size_t)256 << 20;

    // the buffers of ours that the jobs' frames lay in are free again: read on warp_stream and refilled on st, they wait for that stream's
    // synchronisation; else they are reused only by later work on this stream
    void release() {
        for (const Job& j : jobs) if (j.release) (warps_apart ? s->held_release : s->pool).push_back(j.release);
    }

    // Host callers: the staged outputs go down.  A call on its own: behind the warps on the same stream; the synchronisation at the end of the
    // call covers them.  A chunk of the pipelined batch: the area is handed to a downloader thread, which waits (on its own stream) for the warps.
    int download() {
        if (!to_host) return VS_OK;
        std::vector<int> idx(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) idx[j] = jobs[j].i;
        const uint8_t* area = (const uint8_t*)s->batch_out[slot].p;
        if (!threaded_download) { VS_HIP(copy_outputs_down(c, idx, area, dbytes, st)); return VS_OK; }
        if (!s->down_stream) VS_HIP(hipStreamCreateWithFlags(&s->down_stream, hipStreamNonBlocking));
        if (!s->down_ev[slot]) VS_HIP(hipEventCreateWithFlags(&s->down_ev[slot], hipEventDisableTiming));
        VS_HIP(hipEventRecord(s->down_ev[slot], st));
        s->down[slot] = run_async([call = c, idx, area, obytes = dbytes, device = vsi::aligner_device(s->aligner), ds = s->down_stream, ev = s->down_ev[slot]]() -> hipError_t {
            hipError_t e = hipSetDevice(device);
            if (e == hipSuccess) e = hipStreamWaitEvent(ds, ev, 0);
            if (e == hipSuccess) e = copy_outputs_down(call, idx, area, obytes, ds);
            return e != hipSuccess ? e : hipStreamSynchronize(ds);
        });
        return VS_OK;
    }

    // frames of this batch that are still queued move into buffers of our own
    int own_queued() {
        for (auto& f : s->frames) {
            if (f.owned || s->defer_own) continue;
            void* copy = nullptr;
            if (!s->pool.empty()) { copy = s->pool.back(); s->pool.pop_back(); }
            else VS_HIP(vsi::dev_alloc(&copy, fbytes));
            VS_HIP(hipMemcpyAsync(copy, f.ptr, fbytes, hipMemcpyDeviceToDevice, st));
            f.ptr = copy; f.owned = true;
        }
        return VS_OK;
    }
};

// out_mem: where the outputs go.  slot_arg >= 0: a chunk of the pipelined host batch -- its outputs leave through output area `slot_arg` and a
// downloader thread of their own, under the next chunk's compute.  slot_arg < 0: a call on its own (process / process_batch that fits one
// chunk): the copies go onto the handle's stream, nothing to overlap with, no thread.
static int stab_chunk(vs_stabilizer* s, const StabCall& c, int out_mem, int slot_arg) {
    VS_ARG(s && c.frames && c.out && c.has_output && c.out_w && c.out_h && c.n >= 1);
    VS_ARG(c.format != VS_FMT_GRAY8 && vs_format_bits(c.format) != 0);
    VS_ARG(c.w > 0 && c.h > 0 && c.w <= 65535 && c.h <= 65535);
    VS_ARG(c.stride >= 3 * c.w);
    const int w = c.w, h = c.h, crop = s->params.crop_pixels > 0 ? s->params.crop_pixels : 0;
    VS_ARG(w > 2 * crop && h > 2 * crop);
    const int ow = w - 2 * crop, oh = h - 2 * crop, lag = s->params.lag;
    const Delivery dl = delivered_size(w, h, crop, s->cfg);
    VS_ARG(c.n == 1 || (c.frame_stride >= (size_t)(h - 1) * c.stride + (size_t)3 * w && c.out_frame_stride >= (size_t)dl.w * dl.h * 3));
    VS_HIP(hipSetDevice(vsi::aligner_device(s->aligner)));
    if (s->w != w || s->h != h || s->fmt != c.format) {
        // a size change restarts the aligner (alignment.cpp:155).  The reference would go on warping queued frames of the
        // old size with measurements of the new one; here the change starts a new clip, cleanly: queued frames of the
        // old size are dropped and the smoother, the accumulated correction and the frame counter start over.
        stab_drop_frames(s);
        VS_TRY(vs_stabilizer_reset(s));
        s->w = w; s->h = h; s->fmt = c.format; s->frame_bytes = c.fbytes();
    }
    *c.out_w = dl.w; *c.out_h = dl.h;

    const bool to_host = out_mem == VS_MEM_HOST, warps_apart = s->overlap_warps && !to_host;
    hipStream_t st = (hipStream_t)vs_aligner_stream(s->aligner);
    Chunk k{s, c, std::max(slot_arg, 0), slot_arg >= 0, to_host, warps_apart, st, warps_apart ? s->warp_stream : st, crop, ow, oh, dl.w, dl.h, dl.resize};
    const PassPlan pp = plan_passes(s->cfg, lag, s->params.warp_mode);
    k.fill.n = pp.fill; k.db.n = pp.deblur; k.dn.n = pp.denoise; k.fk.n = pp.deflicker; k.rs.n = pp.rolling;
    k.blend_on = pp.blend_on; k.want_sums = pp.want_sums;

    VS_TRY(k.make_dense());
    VS_TRY(k.measure_side_values());
    VS_TRY(k.align());
    VS_TRY(k.detect_cuts());
    VS_TRY(k.frame_loop());
    if (!k.jobs.empty()) {
        VS_TRY(k.passes());
        VS_TRY(k.warp_runs());
        k.release();
        VS_TRY(k.download());
    }
    if (!warps_apart) sharp_settle(s);                    // (readers and the next writer share this stream)
    if (c.clip_len > 0) VS_TRY(vs_stabilizer_reset(s));   // nothing carries over from the last clip
    VS_TRY(k.own_queued());
    VS_TRY(k.keep_last_frame());
    if (!s->prefetched) VS_HIP(hipStreamSynchronize(st));   // (with the next chunk's alignment in flight its completion is the next call's wait)
    return std::accumulate(c.has_output, c.has_output + c.n, 0);
}
// (guarded: an exception inside a chunk -- a host allocation that fails -- comes back as an error code, so that the callers' loops restore
// the handle's modes and stab_run's failure protocol runs)
static int stab_run_impl(vs_stabilizer* s, const StabCall& c, int out_mem, int slot) {
    return vsi::guarded([&] { return stab_chunk(s, c, out_mem, slot); });
}

// The batch split into chunks of `chunk` frames (whole clips in clip mode): an uploader thread fills the other upload area
// with chunk k+1 while chunk k is aligned and warped, and a downloader thread drains chunk k's outputs while chunk k+1 is
// computed -- upload, compute and download overlap, and the link carries input and output at the same time (full duplex).
// Every chunk goes through stab_run_impl exactly as a separate vs_stabilizer_process_batch call would, which is the
// definition of the batched form ("n successive process calls"), so the results do not depend on the chunking.
static int stab_run_host_pipelined(vs_stabilizer* s, const StabCall& c, int chunk) {
    VS_ARG(s && c.frames && c.out && c.has_output && c.out_w && c.out_h);
    VS_ARG(c.w > 0 && c.h > 0 && c.w <= 65535 && c.h <= 65535);
    VS_ARG(c.format != VS_FMT_GRAY8 && vs_format_bits(c.format) != 0 && c.stride >= 3 * c.w);
    VS_ARG(c.frame_stride >= (size_t)(c.h - 1) * c.stride + (size_t)3 * c.w);
    const int device = vsi::aligner_device(s->aligner);
    VS_HIP(hipSetDevice(device));
    VS_HIP(grow(s->pipe_in, &s->pipe_in_bytes, c.fbytes() * chunk, nullptr, false, 2));
    if (!s->up_stream) VS_HIP(hipStreamCreateWithFlags(&s->up_stream, hipStreamNonBlocking));
    const bool dense = c.dense();
    auto upload = [=](int k) -> hipError_t {                 // chunk k -> pipe_in[k & 1], dense
        const int off = k * chunk;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = make_dense(s, c.sub(off, std::min(chunk, c.n - off)), dense, k & 1, s->pipe_in[k & 1], s->up_stream);
        return e != hipSuccess ? e : hipStreamSynchronize(s->up_stream);
    };
    const int n_chunks = (c.n + chunk - 1) / chunk;
    std::future<hipError_t> next = run_async(upload, 0);
    int produced = 0;
    for (int k = 0; k < n_chunks; k++) {
        const int off = k * chunk;
        const hipError_t ue = next.get();
        if (k + 1 < n_chunks) next = run_async(upload, k + 1);
        int r = ue == hipSuccess ? VS_OK : set_error(VS_ERR_HIP, "frame upload failed: %s", hipGetErrorString(ue));
        if (r == VS_OK) r = stab_run_impl(s, c.sub(off, std::min(chunk, c.n - off)).dense_at(s->pipe_in[k & 1]), VS_MEM_HOST, k & 1);
        if (r < 0) { if (next.valid()) (void)next.get(); return r; }
        produced += r;
    }
    return produced;
}

// A dense device-resident batch in sub-batches of `step` frames, the warps on warp_stream: those of sub-batch g run under the alignment of
// sub-batch g + 1 (started early with `prefetch`), which takes solver build `mode`.  Every sub-batch goes through stab_run_impl exactly as a call
// of its own would.  defer: frames still queued at a boundary stay pointers into the caller's batch (it outlives the call) and only the last
// sub-batch copies them out; buffers of earlier calls whose last reader is a warp on warp_stream return to the pool only after that stream's
// synchronisation.
static int stab_run_overlapped(vs_stabilizer* s, const StabCall& c, int step, bool defer, int mode, bool prefetch) {
    vs_aligner* a = s->aligner;
    hipStream_t st = (hipStream_t)vs_aligner_stream(a);
    int r = 0;
    hipError_t he = hipSetDevice(vsi::aligner_device(a));
    if (he == hipSuccess && !s->warp_stream) he = hipStreamCreateWithFlags(&s->warp_stream, hipStreamNonBlocking);
    if (he == hipSuccess && !s->warp_ev) he = hipEventCreateWithFlags(&s->warp_ev, hipEventDisableTiming);
    // whatever the handle's stream was told to wait for (vs_stabilizer_wait_stream) holds for the warps too
    if (he == hipSuccess) he = hipEventRecord(s->warp_ev, st);
    if (he == hipSuccess) he = hipStreamWaitEvent(s->warp_stream, s->warp_ev, 0);
    if (he != hipSuccess) r = set_error(VS_ERR_HIP, "stabilizer warp stream: %s", hipGetErrorString(he));
    const int saved_mode = vsi::aligner_batch_mode(a);
    vsi::aligner_set_batch_mode(a, mode);
    s->overlap_warps = true;
    for (int f0 = 0; r >= 0 && f0 < c.n; f0 += step) {
        const int m = std::min(step, c.n - f0);
        s->defer_own = defer && f0 + m < c.n;
        s->next_n = prefetch ? std::min(step, c.n - f0 - m) : 0;
        s->next_frames = c.frame(f0 + m);
        const int rg = stab_run_impl(s, c.sub(f0, m), c.mem, -1);
        r = rg < 0 ? rg : r + rg;
    }
    s->defer_own = false; s->overlap_warps = false; s->next_n = 0;
    vsi::aligner_set_batch_mode(a, saved_mode);
    const hipError_t we = s->warp_stream ? hipStreamSynchronize(s->warp_stream) : hipSuccess;   // every warp has landed before the call returns
    if (we != hipSuccess && r >= 0) r = set_error(VS_ERR_HIP, "stabilizer warps: %s", hipGetErrorString(we));
    for (void* b : s->held_release) s->pool.push_back(b);
    s->held_release.clear();
    sharp_settle(s);
    return r;
}

// While a batch is in flight the frame queue holds non-owned pointers into the caller's buffer (or into batch_in); they
// become copies of our own only at the end of a successful run.  Whatever stops a run early -- a HIP error, a refused
// warp -- must not leave such an entry behind for the next call to warp from: the stabilizer is reset to a clean
// "new clip" state (and the stream drained, so nothing still reads the caller's frames), and the error is passed on.
static int stab_run(vs_stabilizer* s, const StabCall& c) {
    if (!s) return stab_run_impl(s, c, c.mem, -1);           // (refused there)
    // the lens was calibrated for one frame size: another one is refused before any work, and leaves the handle as it is
    if (s->cfg.lens_on && (c.w != s->cfg.lens_w || c.h != s->cfg.lens_h))
        return set_error(VS_ERR_ARG, "bad argument: lens correction is set for %d x %d frames, this call brings %d x %d (vs_stabilizer_set_lens)", s->cfg.lens_w, s->cfg.lens_h, c.w, c.h);
    // an output size the resize cannot reach from this call's window is refused before any work, and leaves the handle as it is
    const int crop = vsi::stab_crop(s);
    if (c.w > 2 * crop && c.h > 2 * crop && c.w <= 65535 && c.h <= 65535) {
        const Delivery dl = delivered_size(c.w, c.h, crop, s->cfg);
        const int ow = c.w - 2 * crop, oh = c.h - 2 * crop;
        if (dl.resize && !vsr::resize_params_valid(ow, oh, dl.w, dl.h, s->cfg.out_filter)) {
            if (dl.w > vsr::kMaxExtent || dl.h > vsr::kMaxExtent || ow > vsr::kMaxExtent || oh > vsr::kMaxExtent)
                return set_error(VS_ERR_UNSUPPORTED, "output size: windows and delivered frames up to 32767 x 32767 (vs_stabilizer_set_output_size)");
            const bool on_x = !vsr::resize_axis_valid(ow, dl.w, s->cfg.out_filter);
            return set_error(VS_ERR_UNSUPPORTED, "output size: VS_RESIZE_AREA needs delivered <= window <= 8 delivered on the %s axis, the window is %d x %d, the output size %d x %d (vs_stabilizer_set_output_size)",
                             on_x ? "x" : "y", ow, oh, dl.w, dl.h);
        }
    }
    // how the call is cut, its thresholds and the numbers they were measured with: pick_route (vs_stab_plan.hpp)
    const StabRoute route = pick_route(RouteIn{c.mem, c.n, c.clip_len, c.w, c.h, c.fbytes(), c.dense(), s->cfg.lens_on, s->params.warp_mode, vsi::ingest_chunk_bytes()},
                                       stab_knobs());
    int r;
    switch (route.kind) {
    case StabRoute::HostPipelined: r = vsi::guarded([&] { return stab_run_host_pipelined(s, c, route.step); }); break;
    case StabRoute::ClipGroups:
    case StabRoute::TimeChunks: r = stab_run_overlapped(s, c, route.step, route.defer, route.solver_mode, route.prefetch); break;
    default: r = stab_run_impl(s, c, c.mem, -1);
    }
    for (auto& f : s->down) if (f.valid()) {                 // every download has landed before the call returns
        const hipError_t de = f.get();
        if (de != hipSuccess && r >= 0) r = set_error(VS_ERR_HIP, "output download failed: %s", hipGetErrorString(de));
    }
    if (r < 0 && s->aligner) {
        const std::string why = vs_last_error();             // the reset below must not hide the cause
        vsi::align_abandon(s->aligner);                      // (a next chunk's alignment may have been started)
        s->prefetched = false; s->next_n = 0;
        s->lens_map_made = false;                            // (the launch that made the map may be what failed)
        (void)hipStreamSynchronize((hipStream_t)vs_aligner_stream(s->aligner));
        for (auto it = s->frames.begin(); it != s->frames.end();) it = it->owned ? it + 1 : s->frames.erase(it);
        (void)vs_stabilizer_reset(s);
        // (everything is quiet now: the sharpness blocks are referred to by what is still queued, if anything, and by nothing else)
        s->sharp_pending.clear();
        for (auto* b : s->sharp_blocks) b->refs = 0;
        for (auto& f : s->frames) { if (f.sb) ++f.sb->refs; if (f.mb) ++f.mb->refs; }
        set_error(r, "%s", why.c_str());
    }
    return r;
}

extern "C" {

int vs_stabilizer_process_batch(vs_stabilizer* s, const void* frames, size_t frame_stride, int n, int w, int h, int stride,
                                int format, int mem, void* out, size_t out_frame_stride, int32_t* has_output, int* out_w,
                                int* out_h) try {
    return stab_run(s, StabCall{frames, frame_stride, n, 0, w, h, stride, format, mem, out, out_frame_stride, has_output, out_w, out_h});
} VS_CATCH_ALL

int vs_stabilizer_process_clips(vs_stabilizer* s, const void* frames, size_t frame_stride, int n_clips, int frames_per_clip,
                                int w, int h, int stride, int format, int mem, void* out, size_t out_frame_stride,
                                int32_t* has_output, int* out_w, int* out_h) try {
    VS_ARG(n_clips >= 1 && frames_per_clip >= 1 && (long long)n_clips * frames_per_clip <= 0x7fffffff);
    return stab_run(s, StabCall{frames, frame_stride, n_clips * frames_per_clip, frames_per_clip, w, h, stride, format, mem, out, out_frame_stride,
                                has_output, out_w, out_h});
} VS_CATCH_ALL

void* vs_stabilizer_stream(const vs_stabilizer* s) { return s ? vs_aligner_stream(s->aligner) : nullptr; }
int vs_stabilizer_set_select_mode(vs_stabilizer* s, int mode) try {
    VS_ARG(s && s->aligner);
    return vs_aligner_set_select_mode(s->aligner, mode);
} VS_CATCH_ALL
int vs_stabilizer_get_select_mode(const vs_stabilizer* s) try {
    VS_ARG(s && s->aligner);
    return vs_aligner_get_select_mode(s->aligner);
} VS_CATCH_ALL
int vs_stabilizer_set_border_fill(vs_stabilizer* s, int ahead) try {
    VS_ARG(s && ahead >= 0);
    if (s->params.warp_mode != VS_WARP_BILINEAR_CV) return set_error(VS_ERR_UNSUPPORTED, "border fill: VS_WARP_BILINEAR_CV handles only (this one has warp_mode %d)", s->params.warp_mode);
    VS_ARG(ahead <= s->params.lag);
    s->cfg.border_fill = ahead;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_border_fill(const vs_stabilizer* s) try {
    VS_ARG(s);
    return s->cfg.border_fill;
} VS_CATCH_ALL
int vs_stabilizer_set_fill_blend(vs_stabilizer* s, const vs_fill_blend_params* params) try {
    VS_ARG(s);
    if (s->params.warp_mode != VS_WARP_BILINEAR_CV) return set_error(VS_ERR_UNSUPPORTED, "fill blend: VS_WARP_BILINEAR_CV handles only (this one has warp_mode %d)", s->params.warp_mode);
    const vs_fill_blend_params p = params ? *params : vs_fill_blend_params{0, 0};
    VS_ARG(vsi::fill_blend_params_valid(p));
    s->cfg.fill_blend = p;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_fill_blend(const vs_stabilizer* s, vs_fill_blend_params* params) try {
    VS_ARG(s && params);
    *params = s->cfg.fill_blend;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_set_inpaint(vs_stabilizer* s, int on) try {
    VS_ARG(s && (on == 0 || on == 1));
    if (s->params.warp_mode != VS_WARP_BILINEAR_CV) return set_error(VS_ERR_UNSUPPORTED, "inpaint: VS_WARP_BILINEAR_CV handles only (this one has warp_mode %d)", s->params.warp_mode);
    s->cfg.inpaint = on;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_inpaint(const vs_stabilizer* s) try {
    VS_ARG(s);
    return s->cfg.inpaint;
} VS_CATCH_ALL
int vs_stabilizer_set_sharpen(vs_stabilizer* s, const vs_sharpen_params* params) try {
    VS_ARG(s);
    if (s->params.warp_mode != VS_WARP_BILINEAR_CV) return set_error(VS_ERR_UNSUPPORTED, "sharpen: VS_WARP_BILINEAR_CV handles only (this one has warp_mode %d)", s->params.warp_mode);
    if (params) VS_ARG(vsi::sharpen_params_valid(*params));
    s->cfg.sharpen_on = params != nullptr;
    if (params) s->cfg.sharpen = *params;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_sharpen(const vs_stabilizer* s, vs_sharpen_params* params) try {
    VS_ARG(s && params);
    if (s->cfg.sharpen_on) *params = s->cfg.sharpen; else vs_sharpen_params_default(params);
    return s->cfg.sharpen_on ? 1 : 0;
} VS_CATCH_ALL
int vs_stabilizer_set_deblur(vs_stabilizer* s, int ahead, const vs_deblur_params* params) try {
    VS_ARG(s && ahead >= 0 && ahead <= s->params.lag);
    vs_deblur_params p;
    if (params) p = *params; else vs_deblur_params_default(&p);
    VS_ARG(vsi::deblur_params_finite(p.sensitivity, p.max_ratio));
    s->cfg.deblur = ahead;
    s->cfg.deblur_params = p;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_deblur(const vs_stabilizer* s) try {
    VS_ARG(s);
    return s->cfg.deblur;
} VS_CATCH_ALL
int vs_stabilizer_set_denoise(vs_stabilizer* s, int ahead, const vs_denoise_params* params) try {
    VS_ARG(s && ahead >= 0 && ahead <= s->params.lag);
    vs_denoise_params p;
    if (params) p = *params; else vs_denoise_params_default(&p);
    VS_ARG(vsi::denoise_params_valid(p));
    s->cfg.denoise = ahead;
    s->cfg.denoise_params = p;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_set_deflicker(vs_stabilizer* s, int ahead, const vs_deflicker_params* params) try {
    VS_ARG(s && ahead >= 0 && ahead <= s->params.lag);
    vs_deflicker_params p;
    if (params) p = *params; else vs_deflicker_params_default(&p);
    VS_ARG(vsi::deflicker_params_valid(p));
    s->cfg.deflicker = ahead;
    s->cfg.deflicker_params = p;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_deflicker(const vs_stabilizer* s) try {
    VS_ARG(s);
    return s->cfg.deflicker;
} VS_CATCH_ALL
int vs_stabilizer_get_denoise(const vs_stabilizer* s) try {
    VS_ARG(s);
    return s->cfg.denoise;
} VS_CATCH_ALL
int vs_stabilizer_set_rolling_shutter(vs_stabilizer* s, const vs_rolling_params* params) try {
    VS_ARG(s);
    const vs_rolling_params p = params ? *params : vs_rolling_params{0.0};
    VS_ARG(vsi::rolling_params_valid(p));
    s->cfg.rolling = p;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_rolling_shutter(const vs_stabilizer* s, vs_rolling_params* params) try {
    VS_ARG(s && params);
    *params = s->cfg.rolling;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_set_lens(vs_stabilizer* s, const vs_lens_params* params, int w, int h) try {
    VS_ARG(s);
    if (params) {
        VS_ARG(vsl::params_ok(*params) && (params->border == VS_BORDER_CLAMP || params->border == VS_BORDER_CONSTANT));
        VS_ARG(w >= 1 && h >= 1);
        if (w > 32767 || h > 32767) return set_error(VS_ERR_UNSUPPORTED, "lens correction: frames up to 32767 x 32767, as the remap");
    }
    // the map belongs to (params, w, h): dropped here, made again by the next call that needs it (no launch of an earlier call still reads
    // it: every call ends with its stream synchronised)
    VS_HIP(hipSetDevice(vsi::aligner_device(s->aligner)));
    s->lens_map.drop();
    s->lens_map_made = false;
    s->cfg.lens_on = params && !vsl::is_identity(*params);
    if (s->cfg.lens_on) { s->cfg.lens = *params; s->cfg.lens_w = w; s->cfg.lens_h = h; }
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_lens(const vs_stabilizer* s, vs_lens_params* params, int* w, int* h) try {
    VS_ARG(s && params && w && h);
    *w = s->cfg.lens_on ? s->cfg.lens_w : 0; *h = s->cfg.lens_on ? s->cfg.lens_h : 0;
    if (s->cfg.lens_on) *params = s->cfg.lens; else vs_lens_params_default(params, 0, 0);
    return s->cfg.lens_on ? 1 : 0;
} VS_CATCH_ALL
int vs_stabilizer_set_output_size(vs_stabilizer* s, int dw, int dh, int filter) try {
    VS_ARG(s && (filter == VS_RESIZE_LINEAR || filter == VS_RESIZE_AREA));
    VS_ARG((dw == 0 && dh == 0) || (dw == -1 && dh == -1) || (dw >= 1 && dh >= 1));
    if (dw > vsr::kMaxExtent || dh > vsr::kMaxExtent) return set_error(VS_ERR_UNSUPPORTED, "output size: up to 32767 x 32767, as the resize");
    s->cfg.out_w = dw; s->cfg.out_h = dh; s->cfg.out_filter = filter;
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_output_size(const vs_stabilizer* s, int* dw, int* dh, int* filter) try {
    VS_ARG(s && dw && dh && filter);
    *dw = s->cfg.out_w; *dh = s->cfg.out_h; *filter = s->cfg.out_filter;
    return s->cfg.out_w != 0 ? 1 : 0;
} VS_CATCH_ALL
int vs_stabilizer_set_scene_cut(vs_stabilizer* s, const vs_scene_params* params) try {
    VS_ARG(s);
    if (params) VS_ARG(vsi::scene_params_valid(*params));
    s->cfg.scene_on = params != nullptr;
    if (params) s->cfg.scene_params = *params;
    else s->scene_prev_valid = false;                                 // (off: no frame is kept; switched on again, a lag-0 handle starts with the frame after next)
    return VS_OK;
} VS_CATCH_ALL
int vs_stabilizer_get_scene_cut(const vs_stabilizer* s, vs_scene_params* params) try {
    VS_ARG(s && params);
    if (s->cfg.scene_on) *params = s->cfg.scene_params; else vs_scene_params_default(params);
    return s->cfg.scene_on ? 1 : 0;
} VS_CATCH_ALL
int vs_stabilizer_get_scene_cuts(const vs_stabilizer* s, int64_t* frames, int cap) try {
    VS_ARG(s && cap >= 0 && (frames || cap == 0));
    const size_t m = std::min(s->cut_list.size(), (size_t)cap);
    for (size_t k = 0; k < m; k++) frames[k] = s->cut_list[s->cut_list.size() - m + k];
    return (int)std::min<long long>(s->cut_total, 0x7fffffff);
} VS_CATCH_ALL
int vs_stabilizer_wait_stream(vs_stabilizer* s, void* producer_stream) try {
    VS_ARG(s && s->aligner);
    return vs_aligner_wait_stream(s->aligner, producer_stream);
} VS_CATCH_ALL

// forget the clip: the next frame starts a new sequence (device buffers are kept)
int vs_stabilizer_reset(vs_stabilizer* s) try {
    VS_ARG(s);
    VS_HIP(hipSetDevice(vsi::aligner_device(s->aligner)));
    for (auto& f : s->frames) { sharp_unhold(s, f); if (f.owned) s->pool.push_back(f.ptr); }
    s->frames.clear();
    s->measurements.clear();
    s->meas_ok.clear();
    s->meas_cut.clear();
    s->scene_prev_valid = false;
    s->cut_total = 0;
    s->cut_list.clear();
    // (make the new smoother first: if that fails the handle keeps a valid, if stale, one -- never a null pointer for the next call to walk into)
    vs_smoother* fresh = vs_smoother_create(s->params.lag, s->params.smoother_memory, s->params.lambda);
    if (!fresh) return VS_ERR_NOMEM;
    vs_smoother_destroy(s->smoother);
    s->smoother = fresh;
    s->accum = vs_transform{0, 0, 0, 0};
    s->last_meas = vs_transform{0, 0, 0, 0};
    s->last_success = 0;
    s->frame_index = 0;
    return vs_aligner_reset(s->aligner);
} VS_CATCH_ALL

int vs_stabilizer_process(vs_stabilizer* s, const void* frame, int w, int h, int stride, int format, int mem, void* out,
                          int* out_w, int* out_h) try {
    int32_t has = 0;
    int r = vs_stabilizer_process_batch(s, frame, 0, 1, w, h, stride, format, mem, out, 0, &has, out_w, out_h);
    return r < 0 ? r : has;
} VS_CATCH_ALL

void vs_stabilizer_state(const vs_stabilizer* s, vs_transform* last_meas, vs_transform* accum, int* last_success) {
    if (last_meas) *last_meas = s->last_meas;
    if (accum) *accum = s->accum;
    if (last_success) *last_success = s->last_success;
}

}  // extern "C"
