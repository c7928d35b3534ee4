// vs_engine.hip -- engine level of the C ABI: VideoAligner (alignment.cpp:149-704) as a device-resident, batched pipeline
// (VideoStabilizer, stabilizer.cpp:9-117, on top of it: vs_stabilizer.hip).
//
// Design (DESIGN.md "Engine"):
//   * Gray pyramids of every frame of a batch live in HBM in one slab: slot s, level l at
//     pyr + s*pyr_frame + L[l].img_off.  Slot 0 is the carry-over frame of the previous call,
//     slots 1..n are this call's frames, so every stage is ONE launch over all frames.
//   * Odd frames (in sequence order) are keyframes (alignment.hpp:65-66): their keypoint tables
//     (arg-max coordinates + Jacobians, every level) are produced by the fused keyframe kernel.
//   * Every alignment depends on exactly two consecutive frames, so all frame pairs of a batch are
//     solved concurrently: per level one warpdiff launch, one selection step, one gather launch and
//     one persistent Gauss-Newton launch in which a whole workgroup owns a pair and iterates on the
//     device until it converges / diverges / runs out of iterations -- no host round trip per
//     iteration (the reference makes one Halide call per iteration, alignment.cpp:600-668).
//   * The transform algebra inside the loop is fp64 on the device, written exactly as imgproc.cpp.
#include "vs_engine.hpp"
#define VS_ALIGN_PLAN_UNIT
#include "vs_align_plan.hpp"
#include "vs_kernels.hpp"
#include "vs_phase.hpp"
#include "vs_device.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

using vsi::set_error;
using vsi::run_async;
using vsi::align_start;
using vsi::align_finish;
using vsi::align_abandon;
using namespace vsd;

namespace {

struct PairDescPack { PairDesc d[kDirectMaxPairs]; };   // latency mode: the descriptors travel in the kernel arguments

// ---- phase-correlation start value (alignment.cpp:376-387) -----------------------------------------
// detected_shift of the level-2 images scaled by (1 << PhaseLevel) / float(1 << PyramidLevels) becomes the initial TX,TY
// (negated when the current frame is the keyframe), if the response clears the threshold.
__global__ void vs_k_phase_apply(PairState* __restrict__ states, const vsp::Result* __restrict__ res,
                                 const uint8_t* __restrict__ negate, int n_pairs, double threshold, float scale) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    const vsp::Result r = res[q];
    if (r.response > threshold) {
        double tx = r.dx * scale, ty = r.dy * scale;
        if (negate[q]) { tx = -tx; ty = -ty; }
        states[q].T[2] = tx;
        states[q].T[3] = ty;
    }
}

// ---- batched sparse_warpdiff: generators.cpp:646-700 for every (pair, set) ---------------------
__global__ __launch_bounds__(256) void vs_k_warpdiff_batch(const PairState* __restrict__ states,
                                                           const PairDesc* __restrict__ descs,
                                                           const uint8_t* __restrict__ pyr, size_t pyr_frame,
                                                           size_t img_off, int w, int h,
                                                           const uint16_t* __restrict__ lm_tab, size_t lm_frame,
                                                           size_t lm_off, int nt, uint16_t* __restrict__ wd,
                                                           float* __restrict__ wv, size_t wd_pair) {
    const int p = blockIdx.y, set = blockIdx.z;
    const PairState& st = states[p];
    if (st.status != 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const PairDesc d = descs[p];
    const uint8_t* tmpl = pyr + (size_t)d.tmpl_slot * pyr_frame + img_off;
    const uint8_t* key = pyr + (size_t)d.key_slot * pyr_frame + img_off;
    const uint16_t* lm = lm_tab + (size_t)d.key_slot * lm_frame + lm_off + (size_t)set * 2 * nt;
    double T[4] = {st.T[0], st.T[1], st.T[2], st.T[3]};
    float P[4];
    ul_params_sparse(T, w, h, P);
    const uint32_t xy = ((const uint32_t*)lm)[i];           // {x, y} pair of tile i
    int tile_x = min((int)(xy & 0xffffu), w - 1), tile_y = min((int)(xy >> 16), h - 1);
    float ox = (float)tile_x, oy = (float)tile_y;
    float Wx = (1.0f + P[0]) * ox - P[1] * oy + P[2];
    float Wy = P[1] * ox + (1.0f + P[0]) * oy + P[3];
    float v = lanczos_sample_u8(key, w, h, w, Wx, Wy);
    float diff = fabsf(v - (float)tmpl[(size_t)tile_y * w + tile_x]);
    diff = fminf(fmaxf(diff, 0.0f), 65535.0f);
    wd[(size_t)p * wd_pair + (size_t)set * nt + i] = (uint16_t)diff;
    wv[(size_t)p * wd_pair + (size_t)set * nt + i] = v;   // the first Gauss-Newton iteration samples the same point (PointRecs::r0)
}

// ---- gather of the selected keypoints + Jacobians: alignment.cpp:523-546 ------------------------
// The solver reads one compact record per selected point, built once per level (both sets back to
// back: x-set at [0,nsel), y-set at [nsel,2*nsel)):
//   xy  u32    x | y << 16                       (SelectedPixels, alignment.cpp:530-531)
//   tv  f32    float(template(min(x,w-1), min(y,h-1)))   -- constant over the iterations (generators.cpp:554-556)
//   j   float4 the four Jacobian components     (SelectedJacobian, alignment.cpp:532-534)
// a value that is the same in every lane, moved to the scalar registers (see gn_level)
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (T*)(((unsigned long long)hi << 32) | lo);
}

//   r0  f32    tv - (the key frame sampled at the point warped by the transform the level STARTS from): the residual of the
//              first Gauss-Newton iteration.  sparse_warpdiff (generators.cpp:672-697) has just computed exactly that sample
//              for every tile -- same image, same fp32 kernel parameters, same point -- so the first sparse_ica pass
//              (generators.cpp:469-498) takes it from here instead of sampling again; the value is the same bit for bit.
struct PointRecs {
    uint32_t* xy;
    float* tv;
    float4* j;
    float* r0;
};
__device__ __forceinline__ PointRecs pair_recs(uint8_t* recs, size_t recs_pair, int p, int nt_cap) {
    uint8_t* base = recs + (size_t)p * recs_pair;
    PointRecs r;
    r.j = (float4*)base;                                      // 2*nt_cap float4
    r.xy = (uint32_t*)(base + (size_t)2 * nt_cap * 16);       // 2*nt_cap u32
    r.tv = (float*)(base + (size_t)2 * nt_cap * 20);          // 2*nt_cap f32
    r.r0 = (float*)(base + (size_t)2 * nt_cap * 24);          // 2*nt_cap f32
    return r;
}
static_assert(kPointRecBytes == 28, "recs_pair_bytes (vs_align_plan.hpp) sizes the block pair_recs lays out");
__device__ __forceinline__ void write_rec(const PointRecs& rc, int slot, const uint16_t* __restrict__ lm,
                                          const float* __restrict__ jac, int nt, int t, const uint8_t* __restrict__ tmpl,
                                          int w, int h, const float* __restrict__ wv_set) {
    const uint32_t xy = ((const uint32_t*)lm)[t];
    const int px = (int)(xy & 0xffffu), py = (int)(xy >> 16);
    rc.xy[slot] = xy;
    const float tv = (float)tmpl[(size_t)min(py, h - 1) * w + min(px, w - 1)];
    rc.tv[slot] = tv;
    rc.r0[slot] = tv - wv_set[t];
    rc.j[slot] = ((const float4*)jac)[t];
}

__global__ __launch_bounds__(256) void vs_k_gather_selected(const PairState* __restrict__ states,
                                                            const PairDesc* __restrict__ descs,
                                                            const uint8_t* __restrict__ pyr, size_t pyr_frame,
                                                            size_t img_off, int w, int h,
                                                            const uint16_t* __restrict__ lm_tab, size_t lm_frame,
                                                            size_t lm_off, const float* __restrict__ jac_tab,
                                                            size_t jac_frame, size_t jac_off, int nt, int nsel,
                                                            const int32_t* __restrict__ idx, size_t idx_pair,
                                                            const float* __restrict__ wv,
                                                            uint8_t* __restrict__ recs, size_t recs_pair, int nt_cap) {
    const int p = blockIdx.y, set = blockIdx.z;
    if (states[p].status != 1) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nsel) return;
    const PairDesc d = descs[p];
    const uint16_t* lm = lm_tab + (size_t)d.key_slot * lm_frame + lm_off + (size_t)set * 2 * nt;
    const float* jac = jac_tab + (size_t)d.key_slot * jac_frame + jac_off + (size_t)set * 4 * nt;
    const uint8_t* tmpl = pyr + (size_t)d.tmpl_slot * pyr_frame + img_off;
    const int t = idx[(size_t)p * idx_pair + (size_t)set * nt + j];
    write_rec(pair_recs(recs, recs_pair, p, nt_cap), set * nsel + j, lm, jac, nt, t, tmpl, w, h, wv + (size_t)p * idx_pair + (size_t)set * nt);
}

// ---- helper workgroups (latency mode) -------------------------------------------------------------------
// When only a few pairs are in flight, a pair is launched as kCoopGroup workgroups: the leader runs the algorithm as
// always, the others take slices of the one embarrassingly parallel pass of the large levels -- sparse_warpdiff of every
// tile (generators.cpp:646-700), which on one CU is bound by that CU's L1 fill rate (every 4-byte window pulls a
// 128-byte line).  The pass is exact per point and every sum stays with the leader, so the results are bit-identical to
// the one-workgroup launch.
// Protocol (one CoopCtrl per pair in device memory, zeroed at allocation; every launch has a new `epoch`, flags hold the
// epoch they were raised in, so nothing is ever reset): helper g raises arrived[g]; at a shared level the leader hands
// slices to the helpers that have arrived BY THEN (assign[g], nslices, T, then t_ready) and never waits for one that has
// not; a helper writes the packed keys of its slice and raises wd_done[g]; the leader reads all keys into LDS and goes on
// alone.  `abort` releases helpers when the pair ends early.  All waits are bounded.
constexpr int kMaxDevices = 64;              // devices the per-device launch caches index; beyond that they are bypassed
struct CoopLevel {
    int t_ready, nslices, pad[2];
    int assign[kCoopMaxGroup];         // slice number of helper g at this level, -1: not taking part
    int wd_done[kCoopMaxGroup];
    double T[4];                       // the transform the level starts from
};
struct CoopCtrl {
    int arrived[kCoopMaxGroup];
    int abort;
    int pad[15];
    CoopLevel lv[kMaxLevels];
};
constexpr size_t kCoopCtrlBytes = (sizeof(CoopCtrl) + 255) & ~(size_t)255;
// per pair: CoopCtrl | u32 keys[2 * nt_cap] (sparse_warpdiff, packed for the selection) | f32 values[2 * nt_cap] (the samples) |
// f32 template pixels[2 * nt_cap];
// these arrays are only ever touched with sc1 stores and sc1 loads (a line one XCD's L2 kept from a plain access would go stale)
__host__ __device__ inline size_t coop_pair_bytes(int nt_cap) { return kCoopCtrlBytes + (((size_t)nt_cap * 24 + 255) & ~(size_t)255); }

// ---- fused per-pair aligner: every level of alignment.cpp:390-688 in ONE launch ---------------------
struct FusedLevels {
    int levels;
    int w[kMaxLevels], h[kMaxLevels], nt[kMaxLevels], nsel[kMaxLevels], tx[kMaxLevels];
    unsigned long long img_off[kMaxLevels], lm_off[kMaxLevels], jac_off[kMaxLevels];
};

// The per-pair kernels are compiled for two workgroup sizes (vs_align_kernels.inc).  512 threads is the faster shape in
// every configuration measured (fewer waves behind every block barrier: 239 1080p pairs 0.70 -> 0.62 ms, one pair alone
// 0.445 -> 0.40 ms, 952 pairs 2.50 -> 2.09 ms, 119 4K pairs 1.34 -> 1.29 ms although the 20736-tile selection itself is
// slower with half the threads) and takes every level up to kSmallWgTiles tiles; larger levels go to the 1024-thread build.
namespace nt1024 {
constexpr int kGnThreads = 1024, kGnVirt = 1024;
#define VS_GN_FUSED_BOUNDS __launch_bounds__(kGnThreads)
#include "vs_align_kernels.inc"
#undef VS_GN_FUSED_BOUNDS
}  // namespace nt1024
namespace nt512 {
constexpr int kGnThreads = 512, kGnVirt = 512;
#define VS_GN_FUSED_BOUNDS __launch_bounds__(kGnThreads)
#include "vs_align_kernels.inc"
#undef VS_GN_FUSED_BOUNDS
}  // namespace nt512
// Small-footprint build of the fused kernel for full batches (DESIGN.md "co-residency"): 256 hardware threads stand in for the
// 512 of nt512 (virtual threads: bit-identical sums), at most 128 VGPRs (4 waves per SIMD) and ~33 KB of LDS (selection arrays
// of one point set; no staged image) -- the footprint of ONE bgr_image_warp workgroup, so a pair's workgroup moves into a CU as
// soon as one warp workgroup leaves it and the alignment of clip k+1 runs under the warp launch of clip k instead of waiting
// for whole CUs to drain.  Levels whose selection arrays (6 B per tile) exceed 32 KB -- a 4K level 0: 20736 tiles -- select on a
// per-pair global scratch (introselect_block_g), up to 128 * 256 tiles.
namespace nt256v {
constexpr int kGnThreads = 256, kGnVirt = 512;
#define VS_GN_FUSED_BOUNDS __launch_bounds__(kGnThreads, 4)
#include "vs_align_kernels.inc"
#undef VS_GN_FUSED_BOUNDS
}  // namespace nt256v
static_assert(nt512::kGnThreads == kBuildThreads[kBuild512] && nt1024::kGnThreads == kBuildThreads[kBuild1024] &&
              nt256v::kGnThreads == kBuildThreads[kBuild256v], "vs_align_plan.hpp plans with the builds' workgroup sizes");

}  // namespace

VS_BOUNDS_TU(vs_bounds_fetch_engine)

// =================================================================================================
// VideoAligner
// =================================================================================================
namespace {

void free_device(std::initializer_list<void**> ptrs) {
    for (void** p : ptrs) { if (*p) (void)hipFree(*p); *p = nullptr; }
}

// the builds of the level-by-level kernels, indexed like kBuildThreads by wg_build(tiles) (vs_align_plan.hpp)
const decltype(&nt512::vs_k_gn_level) kGnLevelBuilds[2] = {nt512::vs_k_gn_level, nt1024::vs_k_gn_level};
const decltype(&nt512::vs_k_select) kSelectBuilds[2] = {nt512::vs_k_select, nt1024::vs_k_select};
const decltype(&nt512::vs_k_align_pairs) kAlignPairsBuilds[kBuilds] = {nt512::vs_k_align_pairs, nt1024::vs_k_align_pairs, nt256v::vs_k_align_pairs};

// The dynamic-LDS limit belongs to (kernel, device) and is shared by every handle of the process: it is only ever raised, and only when a
// launch needs more than was granted before (the call costs microseconds of host time).  slot: the kernel's row in the cache.
enum { kDynAlignPairs = 0, kDynSelect = kBuilds, kDynSlots = kBuilds + 2 };
int raise_dyn_lds(const void* kernel, int slot, int device, size_t bytes) {
    static std::mutex dyn_mu;
    static size_t dyn_set[kDynSlots][kMaxDevices];
    std::lock_guard<std::mutex> g(dyn_mu);
    size_t& granted = dyn_set[slot][std::min(std::max(device, 0), kMaxDevices - 1)];
    if (granted < bytes || device >= kMaxDevices) {
        VS_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(bytes, granted)));
        granted = std::max(bytes, granted);
    }
    return VS_OK;
}

}  // namespace

struct vs_aligner : LevelTable {          // the level table of the configured size: levels, L[], pyr_frame, lm_frame, jac_frame, nt_max
    int device = 0;
    hipStream_t stream = nullptr;
    vs_aligner_params params;
    int select_mode = VS_SELECT_DEVICE;   // same survivors in the same order as the host path (tests/test_select_gpu.py)
    int batch_mode = VS_BATCH_EXCLUSIVE;  // VS_BATCH_SHARED: full batches through the small-footprint solver kernel
    int cu_count = kChipCUs;              // hipDeviceProp_t::multiProcessorCount of `device` (vs_aligner_create)
    bool coop_ok = true;                  // helper workgroups: only on the architecture their sc1 hand-offs were validated on (gfx950)

    // sequence state (alignment.hpp:61-70)
    int W = -1, H = -1, fmt = -1;
    long long seq = 0;          // frames consumed since (re)initialisation
    int clip_len = 0;           // > 0 during vs_aligner_align_clips: the batch is independent clips of this many frames

    // device storage
    int cap = 0;                // frames per internal chunk (slots = cap + 1)
    uint8_t* pyr = nullptr;
    uint16_t* lm = nullptr;
    float* jac = nullptr;
    PairState* states = nullptr;
    PairDesc* descs = nullptr;
    uint16_t* wd = nullptr;
    float* wv = nullptr;          // per pair: the 2*nt_max sparse_warpdiff samples of the current level (-> PointRecs::r0); fused kernel: + the template pixels
    int32_t* idx = nullptr;
    uint8_t* recs = nullptr;      // per pair: float4 j[2*nt_max] | u32 xy[2*nt_max] | f32 tv[2*nt_max]
    uint8_t* coop = nullptr;      // helper-workgroup control blocks + exchange buffers (kCoopMaxPairs pairs), see CoopCtrl
    void* selbuf = nullptr; size_t selbuf_bytes = 0;   // small-footprint solver: per pair u32 keys[nt_max] | u16 ranks[nt_max] (levels that do not fit its LDS)
    int coop_epoch = 0;
    void* stage = nullptr; size_t stage_bytes = 0;   // host-frame upload area (single chunk)
    // host-resident video: two upload areas filled alternately by an uploader thread on its own stream, so the
    // upload of chunk c+1 runs under the pipeline of chunk c (alignment.cpp:210-218: every frame arrives as a host cv::Mat)
    void* ingest[2] = {nullptr, nullptr}; size_t ingest_bytes = 0;
    hipStream_t copy_stream = nullptr;
    // phase-correlation mode (allocated on first use): level-2 half spectra per slot, per-pair scratch and results
    vsp::Context phase;
    int phase_cap = 0;
    float2* pspec = nullptr;
    float2* pG = nullptr;
    float* psurf = nullptr;
    vsp::Pair* ppairs = nullptr;
    uint8_t* pneg = nullptr;
    vsp::Result* pres = nullptr;
    std::vector<vsp::Result> h_pres;
    // pinned host mirrors
    uint16_t* h_wd = nullptr;
    int32_t* h_idx = nullptr;
    PairState* h_states = nullptr;
    PairDesc* h_descs = nullptr;   // pinned: the descriptor upload needs no host synchronisation before the launch

    std::vector<vs_align_info> info;   // last call
    int last_n = 0;

    // opt-in stage timing (alignment.cpp:10-147's PerformanceMetrics)
    bool timing = false;
    vs_stage_timings tm{};
    struct Span { int stage; hipEvent_t a, b; };
    std::vector<Span> spans;               // open spans of the current chunk
    std::vector<hipEvent_t> event_pool;
    hipEvent_t get_event() {
        if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
        hipEvent_t e; (void)hipEventCreate(&e); return e;
    }
    void t_begin(int stage) {
        if (!timing) return;
        Span sp{stage, get_event(), get_event()};
        (void)hipEventRecord(sp.a, stream);
        spans.push_back(sp);
    }
    void t_end(int launches) {
        if (!timing) return;
        (void)hipEventRecord(spans.back().b, stream);
        tm.launches[spans.back().stage] += launches;
    }
    void t_collect() {   // call after a stream sync
        for (Span& sp : spans) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) tm.ms[sp.stage] += ms;
            event_pool.push_back(sp.a); event_pool.push_back(sp.b);
        }
        spans.clear();
    }

    ~vs_aligner() {
        release();
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        if (stream) { (void)vsi::retire_stream(stream); (void)hipStreamDestroy(stream); }   // (the stabilizer warps on this stream)
    }
    void release();
    int configure(int w, int h, int format, const vs_aligner_params& p);
    int ensure_capacity(int n);
    int ensure_phase();
    void release_phase_buffers();
    void release_phase() { release_phase_buffers(); phase.destroy(); }
    // One chunk = chunk_begin (everything up to and including the solver launch and the copy of its results towards the host: no
    // host synchronisation unless phase correlation is on) + chunk_end (wait, the rare host redo, conversion of the results).
    // run_chunk is the two back to back; the stabilizer puts a chunk's host work between the next chunk's begin and end.
    struct Chunk {
        bool open = false;
        int n = 0, epoch = 0;
        vs_aligner_params p;
        vs_transform* out = nullptr; int32_t* status = nullptr; vs_align_info* infos = nullptr;
        ChunkFrames fr;      // sequence indices, keyframes, pairs
        SolverPlan plan;     // how the pairs are solved
    } ck;
    int chunk_begin(const void* frames, size_t frame_stride, int n, int stride, int mem, const vs_aligner_params& p,
                    vs_transform* out, int32_t* status, vs_align_info* infos);
    int chunk_end();
    int run_chunk(const void* frames, size_t frame_stride, int n, int stride, int mem, const vs_aligner_params& p,
                  vs_transform* out, int32_t* status, vs_align_info* infos) {
        VS_TRY(chunk_begin(frames, frame_stride, n, stride, mem, p, out, status, infos));
        return chunk_end();
    }
    // the steps of chunk_begin, in stream order ...
    int carry_over(uint8_t* dst_pyr, uint16_t* dst_lm, float* dst_jac);
    int ingest_frames(const void* frames, size_t frame_stride, int stride, int mem);
    int phase_spectra();
    int keyframes();
    int start_pairs();
    int phase_start_values();
    int launch_solver();
    // ... and of chunk_end
    int wait_solver();
    int host_redo();
    void convert_results();
    void reset_states(int n_pairs) {
        for (int q = 0; q < n_pairs; q++) { memset(&h_states[q], 0, sizeof(PairState)); h_states[q].status = 1; }
    }
    int launch_phase_apply();
    int select_host(int n_pairs, const LevelDims& l);
    // vs_aligner_align_batch / _clips in two halves (single-chunk device-resident batches run asynchronously in between; anything
    // else completes inside align_start)
    bool started = false, started_clips = false;
    int started_n = 0, started_result = 0;
    int32_t* started_status = nullptr;
};

void vs_aligner::release_phase_buffers() {
    free_device({(void**)&pspec, (void**)&pG, (void**)&psurf, (void**)&ppairs, (void**)&pneg, (void**)&pres});
    phase_cap = 0;
}

// buffers of the phase-correlation mode for the current chunk capacity (PhaseLevel = 2, alignment.hpp:69)
int vs_aligner::ensure_phase() {
    const LevelDims& pl = L[2];
    if (phase.w != pl.w || phase.h != pl.h) {
        release_phase();
        const hipError_t pe = phase.configure(pl.w, pl.h, stream);
        if (pe == hipErrorInvalidValue)
            return set_error(VS_ERR_UNSUPPORTED, "phase_correlate: level 2 is %dx%d, padded extent over %d", pl.w, pl.h, vsp::kMaxLine);
        VS_HIP(pe);                                     // (a refused allocation or a failed upload is a HIP error, not a size problem)
    }
    if (phase_cap >= cap) return VS_OK;
    release_phase_buffers();
    VS_HIP(vsi::dev_alloc((void**)&pspec, ((size_t)cap + 1) * phase.spec_frame() * sizeof(float2)));
    VS_HIP(vsi::dev_alloc((void**)&pG, (size_t)cap * phase.spec_frame() * sizeof(float2)));
    VS_HIP(vsi::dev_alloc((void**)&psurf, (size_t)cap * phase.surface_elems() * sizeof(float)));
    VS_HIP(vsi::dev_alloc((void**)&ppairs, (size_t)cap * sizeof(vsp::Pair)));
    VS_HIP(vsi::dev_alloc((void**)&pneg, (size_t)cap));
    VS_HIP(vsi::dev_alloc((void**)&pres, (size_t)cap * sizeof(vsp::Result)));
    phase_cap = cap;
    return VS_OK;
}

void vs_aligner::release() {
    release_phase();
    free_device({(void**)&pyr, (void**)&lm, (void**)&jac, (void**)&states, (void**)&descs, (void**)&wd, (void**)&wv, (void**)&idx,
                 (void**)&recs, (void**)&coop, &stage, &ingest[0], &ingest[1], &selbuf});
    stage_bytes = 0; ingest_bytes = 0; selbuf_bytes = 0;
    for (void** p : {(void**)&h_wd, (void**)&h_idx, (void**)&h_states, (void**)&h_descs}) { if (*p) (void)hipHostFree(*p); *p = nullptr; }
    cap = 0;
}

// alignment.cpp:155-204: (re)initialisation on first use or size change.  The size is validated BEFORE anything of the old configuration is
// released or overwritten: a refused size leaves the handle exactly as it was (the reference marks a failed setup with LastWidth = -1,
// alignment.cpp:360)
int vs_aligner::configure(int w, int h, int format, const vs_aligner_params& p) {
    LevelTable t;
    VS_TRY(build_levels(w, h, p, &t));
    release();
    static_cast<LevelTable&>(*this) = t;
    W = w; H = h; fmt = format; seq = 0;
    return VS_OK;
}

// the previous chunk's last frame (slot last_n: pyramid + keyframe tables) becomes slot 0 of the slabs at dst_*
int vs_aligner::carry_over(uint8_t* dst_pyr, uint16_t* dst_lm, float* dst_jac) {
    VS_HIP(hipMemcpyAsync(dst_pyr, pyr + (size_t)last_n * pyr_frame, pyr_frame, hipMemcpyDeviceToDevice, stream));
    VS_HIP(hipMemcpyAsync(dst_lm, lm + (size_t)last_n * lm_frame, lm_frame * 2, hipMemcpyDeviceToDevice, stream));
    VS_HIP(hipMemcpyAsync(dst_jac, jac + (size_t)last_n * jac_frame, jac_frame * 4, hipMemcpyDeviceToDevice, stream));
    return VS_OK;
}

// Grows the per-chunk storage to n frames: allocate the whole new set -> copy the carry-over frame -> swap -> free the old set.
// Any failure on the way frees what was allocated here and leaves the handle exactly as it was (same buffers, same `cap`, the
// carry-over frame where it sat), so a failed call is simply a failed call: the next one -- after the caller has made room, or with
// a smaller batch -- finds a consistent handle (tests/test_alloc_failure_gpu.py walks a failure over every allocation).
int vs_aligner::ensure_capacity(int n) {
    if (n <= cap) return VS_OK;
    const int newcap = n;
    const size_t slots = (size_t)newcap + 1;
    const size_t coop_bytes = std::min(newcap, kCoopMaxPairs) * coop_pair_bytes(nt_max);
    // the new set; `owned` frees whatever is still in it when this function returns early
    struct NewSet {
        void* dev[10] = {};
        void* pinned[4] = {};
        ~NewSet() {
            for (void* q : dev) if (q) (void)hipFree(q);
            for (void* q : pinned) if (q) (void)hipHostFree(q);
        }
    } ns;
    enum { D_PYR, D_LM, D_JAC, D_STATES, D_DESCS, D_WD, D_IDX, D_WV, D_RECS, D_COOP };
    const size_t dev_bytes[10] = {
        slots * pyr_frame, slots * lm_frame * 2, slots * jac_frame * 4, sizeof(PairState) * newcap, sizeof(PairDesc) * newcap,
        (size_t)newcap * 2 * nt_max * sizeof(uint16_t), (size_t)newcap * 2 * nt_max * sizeof(int32_t),
        (size_t)newcap * 2 * nt_max * sizeof(float) * 2,      // samples of all pairs, then template pixels
        (size_t)newcap * recs_pair_bytes(nt_max), coop_bytes};
    const size_t pinned_bytes[4] = {dev_bytes[D_WD], dev_bytes[D_IDX], dev_bytes[D_STATES], dev_bytes[D_DESCS]};   // the host mirrors
    for (int i = 0; i < 10; i++) VS_HIP(vsi::dev_alloc(&ns.dev[i], dev_bytes[i]));
    for (int i = 0; i < 4; i++) VS_HIP(vsi::pinned_alloc(&ns.pinned[i], pinned_bytes[i]));
    VS_HIP(hipMemsetAsync(ns.dev[D_COOP], 0, coop_bytes, stream));
    const bool carry = pyr && seq > 0;
    if (carry) VS_TRY(carry_over((uint8_t*)ns.dev[D_PYR], (uint16_t*)ns.dev[D_LM], (float*)ns.dev[D_JAC]));
    VS_HIP(hipStreamSynchronize(stream));        // nothing reads the old set any more; nothing below can fail
    // ---- swap: the handle takes the new set, `ns` takes the old one and frees it on the way out ----
    void** dev_members[10] = {(void**)&pyr, (void**)&lm, (void**)&jac, (void**)&states, (void**)&descs, (void**)&wd, (void**)&idx,
                              (void**)&wv, (void**)&recs, (void**)&coop};
    void** pinned_members[4] = {(void**)&h_wd, (void**)&h_idx, (void**)&h_states, (void**)&h_descs};
    for (int i = 0; i < 10; i++) std::swap(*dev_members[i], ns.dev[i]);
    for (int i = 0; i < 4; i++) std::swap(*pinned_members[i], ns.pinned[i]);
    if (carry) last_n = 0;                       // the carry-over now lives in slot 0
    coop_epoch = 0;
    cap = newcap;
    return VS_OK;
}

// alignment.cpp:435-492: flatten row-major, std::nth_element on abs_delta, keep the first n.
// This IS the reference's selection (same STL call on the same element type and order), run on the
// host for every (pair, set) of the batch, spread over a few threads.
int vs_aligner::select_host(int n_pairs, const LevelDims& l) {
    struct DeltaPixel { uint16_t abs_delta, tile_x, tile_y; };   // alignment.hpp:84-87
    const int nt = l.nt, nsel = l.nsel, tx = l.tx;
    const size_t wd_pair = (size_t)2 * nt_max;
    auto work = [&](int begin, int end) {
        std::vector<DeltaPixel> v;
        for (int job = begin; job < end; job++) {
            const int p = job >> 1, set = job & 1;
            if (h_states[p].status != 1) continue;
            const uint16_t* src = h_wd + (size_t)p * wd_pair + (size_t)set * nt;
            if (select_mode == VS_SELECT_STABLE) {
                // (levels beyond the on-device capacity in VS_SELECT_STABLE mode: the same rule on the host --
                // smallest by (abs_delta, tile index), survivors in tile order)
                std::vector<uint64_t> key((size_t)nt);
                for (int i = 0; i < nt; i++) key[i] = ((uint64_t)src[i] << 32) | (uint32_t)i;
                std::vector<uint64_t> sorted(key);
                int32_t* dst = h_idx + (size_t)p * wd_pair + (size_t)set * nt;
                if (nsel > 0) {
                    std::nth_element(sorted.begin(), sorted.begin() + (nsel - 1), sorted.end());     // (distinct keys: the cut is unique)
                    const uint64_t cut = sorted[nsel - 1];
                    int m = 0;
                    for (int i = 0; i < nt; i++) if (key[i] <= cut) dst[m++] = i;
                }
                continue;
            }
            v.clear();
            v.reserve(nt);
            for (int j = 0; j < l.ty; j++)
                for (int k = 0; k < tx; k++)
                    v.push_back(DeltaPixel{src[(size_t)j * tx + k], (uint16_t)k, (uint16_t)j});
            std::nth_element(v.begin(), v.begin() + nsel, v.end(),
                             [](const DeltaPixel& a, const DeltaPixel& b) { return a.abs_delta < b.abs_delta; });
            int32_t* dst = h_idx + (size_t)p * wd_pair + (size_t)set * nt;
            for (int j = 0; j < nsel; j++) dst[j] = (int32_t)v[j].tile_y * tx + v[j].tile_x;
        }
    };
    const int jobs = n_pairs * 2;
    int nthreads = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
    nthreads = std::min(nthreads, std::max(1, jobs / 8));
    if (nthreads <= 1) {
        work(0, jobs);
    } else {
        std::vector<std::thread> th;
        const int per = (jobs + nthreads - 1) / nthreads;
        for (int t = 0; t < nthreads; t++) {
            int b = t * per, e = std::min(jobs, b + per);
            if (b < e) th.emplace_back(work, b, e);
        }
        for (auto& t : th) t.join();
    }
    return VS_OK;
}

// ---- ComputePyramid (alignment.cpp:149-235) for all n frames: upload, gray levels 0 and 1, the coarser levels ----
int vs_aligner::ingest_frames(const void* frames, size_t frame_stride, int stride, int mem) {
    hipStream_t s = stream;
    const int n = ck.n, ch = fmt == VS_FMT_GRAY8 ? 1 : 3, fbits = vs_format_bits(fmt);
    const size_t esz = fbits > 8 ? 2 : 1;
    const void* dframes = frames;
    t_begin(VS_STAGE_INGEST);
    if (mem == VS_MEM_HOST) {
        const size_t bytes = ((size_t)(n - 1) * frame_stride + (size_t)(H - 1) * stride + (size_t)W * ch) * esz;
        VS_HIP(vsi::grow(&stage, &stage_bytes, bytes));
        VS_HIP(hipMemcpyAsync(stage, frames, bytes, hipMemcpyHostToDevice, s));
        dframes = stage;
    }
    uint8_t* slot1 = pyr + pyr_frame;   // level 0 of slot 1
    if (fmt == VS_FMT_GRAY8) {
        for (int i = 0; i < n; i++)
            VS_HIP(hipMemcpy2DAsync(slot1 + (size_t)i * pyr_frame, W, (const uint8_t*)dframes + (size_t)i * frame_stride,
                                    stride, W, H, hipMemcpyDeviceToDevice, s));
    } else {
        // BGR -> gray level 0 and level 1 in one pass (levels >= 3 always, so level 1 exists)
        VS_HIP(vsk::ingest_pyr(dframes, W, H, stride, fbits > 8 ? 16 : 8, fbits - 8, slot1,
                               slot1 + L[1].img_off, n, frame_stride, pyr_frame, s));
    }
    t_end(1);
    t_begin(VS_STAGE_PYR_DOWN);
    for (int l = (fmt == VS_FMT_GRAY8 ? 1 : 2); l < levels; l++)
        VS_HIP(vsk::pyr_down(slot1 + L[l - 1].img_off, L[l - 1].w, L[l - 1].h, L[l - 1].w, slot1 + L[l].img_off, L[l].w,
                             L[l].h, L[l].w, n, pyr_frame, pyr_frame, s));
    t_end(levels - (fmt == VS_FMT_GRAY8 ? 1 : 2));
    return VS_OK;
}

// ---- PhaseImage (alignment.cpp:225-229): half spectra of level 2, for the carry-over slot too ------------
int vs_aligner::phase_spectra() {
    VS_TRY(ensure_phase());
    t_begin(VS_STAGE_PHASE);
    const int first = (seq > 0 && clip_len == 0) ? 0 : 1;
    VS_HIP(phase.spectra(pyr + (size_t)first * pyr_frame + L[2].img_off, pyr_frame, L[2].w, ck.n + 1 - first,
                         pspec + (size_t)first * phase.spec_frame(), stream));
    t_end(2);
    return VS_OK;
}

// ---- ComputeKeyFrame (alignment.cpp:237-276) for the odd frames of the sequence -----------
int vs_aligner::keyframes() {
    hipStream_t s = stream;
    if (ck.fr.key_runs.empty()) return VS_OK;
    t_begin(VS_STAGE_KEYFRAME);
    int kf_launches = 0;
    for (const std::pair<int, int>& r : ck.fr.key_runs) {
        const int n_odd = r.second;
        const size_t so = (size_t)(r.first + 1);
        vsk::KeyframeLevels KL{};
        KL.n = levels;
        for (int l = 0; l < levels; l++)
            KL.lv[l] = vsk::KeyframeLevel{L[l].w, L[l].h, L[l].ts, L[l].tx, L[l].ty, 0, 0, L[l].img_off, L[l].lm_off, L[l].jac_off};
        if (vsk::keyframe_levels_supported(KL)) {
            // one launch for every level of every keyframe of the run
            VS_HIP(vsk::keyframe_levels(pyr + so * pyr_frame, lm + so * lm_frame, jac + so * jac_frame, KL, n_odd, 2 * pyr_frame,
                                        2 * lm_frame, 2 * jac_frame, s));
            kf_launches += 1;
        } else {
            for (int l = 0; l < levels; l++) {
                uint16_t* lmx = lm + so * lm_frame + L[l].lm_off;
                float* jx = jac + so * jac_frame + L[l].jac_off;
                VS_HIP(vsk::keyframe(pyr + so * pyr_frame + L[l].img_off, L[l].w, L[l].h, L[l].w, L[l].ts, lmx,
                                     lmx + 2 * (size_t)L[l].nt, jx, jx + 4 * (size_t)L[l].nt, n_odd, 2 * pyr_frame,
                                     2 * lm_frame, 2 * jac_frame, s, true));
            }
            kf_launches += levels;
        }
    }
    t_end(kf_launches);
    return VS_OK;
}

// ---- frame pairs: empty results for every frame, then the descriptors and start states of the pairs ----
// (the descriptors and the start states come from pinned memory that is not touched again before the final synchronisation of this
// call: no host synchronisation in front of the launch -- it would expose the launch latency)
int vs_aligner::start_pairs() {
    for (int i = 0; i < ck.n; i++) {
        memset(&ck.infos[i], 0, sizeof(vs_align_info));
        ck.infos[i].levels = levels;
        ck.out[i] = vs_transform{0, 0, 0, 0};
        ck.status[i] = 0;
        if (ck.fr.first(i)) ck.infos[i].fail_reason = 1;
    }
    const int n_pairs = ck.fr.n_pairs();
    ck.plan = SolverPlan{};
    if (n_pairs == 0) return VS_OK;
    ck.plan = plan_solver(*this, n_pairs, cap, ck.p, select_mode, batch_mode, cu_count, coop_ok, solver_knobs());
    for (int q = 0; q < n_pairs; q++) h_descs[q] = ck.fr.desc(q);
    reset_states(n_pairs);
    if (!ck.plan.direct) {
        VS_HIP(hipMemcpyAsync(descs, h_descs, sizeof(PairDesc) * n_pairs, hipMemcpyHostToDevice, stream));
        VS_HIP(hipMemcpyAsync(states, h_states, sizeof(PairState) * n_pairs, hipMemcpyHostToDevice, stream));
    }
    return VS_OK;
}

// detected_shift of the level-2 images scaled by (1 << PhaseLevel) / float(1 << PyramidLevels) becomes the start TX,TY of every pair
int vs_aligner::launch_phase_apply() {
    const int n_pairs = ck.fr.n_pairs();
    const float phase_scale = (1 << 2) / float(1 << levels);
    hipLaunchKernelGGL(vs_k_phase_apply, dim3((n_pairs + 255) / 256), dim3(256), 0, stream, states, pres, pneg, n_pairs,
                       ck.p.phase_correlate_threshold, phase_scale);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// alignment.cpp:369-388: cv::phaseCorrelate(PhaseImage[Prev], PhaseImage[Curr]) starts TX,TY of every pair
int vs_aligner::phase_start_values() {
    hipStream_t s = stream;
    const int n_pairs = ck.fr.n_pairs();
    std::vector<vsp::Pair> hp(n_pairs);
    std::vector<uint8_t> hneg(n_pairs);
    for (int q = 0; q < n_pairs; q++) {
        const int i = ck.fr.pair_frame[q];
        hp[q] = vsp::Pair{i, i + 1};
        hneg[q] = ck.fr.negate(q) ? 1 : 0;
    }
    VS_HIP(hipMemcpyAsync(ppairs, hp.data(), sizeof(vsp::Pair) * n_pairs, hipMemcpyHostToDevice, s));
    VS_HIP(hipMemcpyAsync(pneg, hneg.data(), (size_t)n_pairs, hipMemcpyHostToDevice, s));
    t_begin(VS_STAGE_PHASE);
    VS_HIP(phase.correlate(pspec, ppairs, n_pairs, pG, psurf, pres, s));
    VS_TRY(launch_phase_apply());
    t_end(4);
    h_pres.resize(n_pairs);
    VS_HIP(hipMemcpyAsync(h_pres.data(), pres, sizeof(vsp::Result) * n_pairs, hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));   // hp, hneg go out of use
    return VS_OK;
}

// VS_SELECT_DEVICE / VS_SELECT_STABLE: every level of every pair in one launch (selection = on-device introselect), as ck.plan has it
int vs_aligner::launch_solver() {
    hipStream_t s = stream;
    const SolverPlan& pl = ck.plan;
    const int n_pairs = ck.fr.n_pairs();
    FusedLevels fl;
    fl.levels = levels;
    for (int l = 0; l < levels; l++) {
        fl.w[l] = L[l].w; fl.h[l] = L[l].h; fl.nt[l] = L[l].nt; fl.nsel[l] = L[l].nsel; fl.tx[l] = L[l].tx;
        fl.img_off[l] = L[l].img_off; fl.lm_off[l] = L[l].lm_off; fl.jac_off[l] = L[l].jac_off;
    }
    if (pl.cores) VS_HIP(vsi::grow(&selbuf, &selbuf_bytes, pl.selbuf_bytes));
    const auto kernel = kAlignPairsBuilds[pl.build];
    VS_TRY(raise_dyn_lds((const void*)kernel, kDynAlignPairs + pl.build, device, pl.dyn));
    t_begin(VS_STAGE_GN);
    ck.epoch = ++coop_epoch;
    PairDescPack dpack{};
    if (pl.direct) for (int q = 0; q < n_pairs; q++) dpack.d[q] = h_descs[q];
    hipLaunchKernelGGL(kernel, dim3(n_pairs * pl.group), dim3(pl.threads), pl.dyn, s,
                       pl.direct ? h_states : states, descs, pyr, pyr_frame, lm, lm_frame, jac, jac_frame, recs, pl.recs_pair, nt_max, (int)pl.dyn,
                       fl, pl.gp, pl.group, coop, ck.epoch, wv, dpack, pl.direct ? 1 : 0, pl.cores ? (uint8_t*)selbuf : nullptr, pl.selbuf_pair);
    VS_HIP(hipGetLastError());
    t_end(1);
    if (!pl.direct) VS_HIP(hipMemcpyAsync(h_states, states, sizeof(PairState) * n_pairs, hipMemcpyDeviceToHost, s));
    return VS_OK;
}

// One chunk (n <= cap frames): the result of n successive AlignNextFrame calls.
int vs_aligner::chunk_begin(const void* frames, size_t frame_stride, int n, int stride, int mem,
                            const vs_aligner_params& p, vs_transform* out, int32_t* status, vs_align_info* infos) {
    if (ck.open) return set_error(VS_ERR_ARG, "a chunk is already in flight on this handle");
    ck.n = n; ck.p = p; ck.out = out; ck.status = status; ck.infos = infos;
    ck.fr.assign(seq, clip_len, n);
    if (seq > 0 && last_n != 0) VS_TRY(carry_over(pyr, lm, jac));
    VS_TRY(ingest_frames(frames, frame_stride, stride, mem));
    if (p.phase_correlate) VS_TRY(phase_spectra());
    VS_TRY(keyframes());
    VS_TRY(start_pairs());
    if (ck.fr.n_pairs() > 0) {
        if (p.phase_correlate) VS_TRY(phase_start_values());
        if (!ck.plan.use_host) VS_TRY(launch_solver());
    }
    ck.open = true;
    return VS_OK;
}

// The fused launch's results reach the host.
int vs_aligner::wait_solver() {
    const int n_pairs = ck.fr.n_pairs();
    if (!(ck.plan.direct && solver_knobs().poll && !timing)) { VS_HIP(hipStreamSynchronize(stream)); return VS_OK; }
    // the kernel writes a pair's `pad` word last, behind a system-scope fence: the results are in host memory when
    // every pair's word has arrived -- the host spins on them instead of sleeping in the runtime (the stream itself
    // is ordered by the next enqueue); after ~2 ms it falls back to the synchronisation, which also reports faults
    const auto t0 = std::chrono::steady_clock::now();
    bool all = false;
    while (!all) {
        all = true;
        for (int q = 0; q < n_pairs; q++)
            if (reinterpret_cast<volatile int32_t*>(&h_states[q].pad)[0] != (int32_t)ck.epoch) { all = false; break; }
        if (!all && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!all) VS_HIP(hipStreamSynchronize(stream));
    else {
        // the results are in; helper workgroups may still be winding down, and a fault in any of them must be this
        // call's error, not the next one's: one non-blocking look at the stream
        const hipError_t qe = hipStreamQuery(stream);
        if (qe != hipSuccess && qe != hipErrorNotReady) VS_HIP(qe);
    }
    return VS_OK;
}

// The level-by-level form with the selection on the host: per level one warpdiff launch, select_host, one gather launch and one
// persistent Gauss-Newton launch.
int vs_aligner::host_redo() {
    hipStream_t s = stream;
    const int n_pairs = ck.fr.n_pairs();
    const size_t wd_pair = (size_t)2 * nt_max, recs_pair = ck.plan.recs_pair;
    const int build = wg_build(nt_max);
    for (int l = levels - 1; l >= 0; l--) {
        const LevelDims& ld = L[l];
        t_begin(VS_STAGE_WARPDIFF);
        hipLaunchKernelGGL(vs_k_warpdiff_batch, dim3((ld.nt + 255) / 256, n_pairs, 2), dim3(256), 0, s, states, descs, pyr,
                           pyr_frame, ld.img_off, ld.w, ld.h, lm, lm_frame, ld.lm_off, ld.nt, wd, wv, wd_pair);
        VS_HIP(hipGetLastError());
        t_end(1);
        {
            const auto t0 = std::chrono::steady_clock::now();
            VS_HIP(hipMemcpyAsync(h_wd, wd, (size_t)n_pairs * wd_pair * 2, hipMemcpyDeviceToHost, s));
            VS_HIP(hipMemcpyAsync(h_states, states, sizeof(PairState) * n_pairs, hipMemcpyDeviceToHost, s));
            VS_HIP(hipStreamSynchronize(s));
            VS_TRY(select_host(n_pairs, ld));
            VS_HIP(hipMemcpyAsync(idx, h_idx, (size_t)n_pairs * wd_pair * 4, hipMemcpyHostToDevice, s));
            if (timing) tm.ms[VS_STAGE_SELECT] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (ld.nsel > 0) {
            t_begin(VS_STAGE_GATHER);
            hipLaunchKernelGGL(vs_k_gather_selected, dim3((ld.nsel + 255) / 256, n_pairs, 2), dim3(256), 0, s, states,
                               descs, pyr, pyr_frame, ld.img_off, ld.w, ld.h, lm, lm_frame, ld.lm_off, jac, jac_frame,
                               ld.jac_off, ld.nt, ld.nsel, idx, wd_pair, wv, recs, recs_pair, nt_max);
            VS_HIP(hipGetLastError());
            t_end(1);
        }
        t_begin(VS_STAGE_GN);
        hipLaunchKernelGGL(kGnLevelBuilds[build], dim3(n_pairs), dim3(kBuildThreads[build]), 0, s, states, descs, pyr, pyr_frame,
                           ld.img_off, ld.w, ld.h, ld.nsel, recs, recs_pair, nt_max, l, ck.plan.gp);
        VS_HIP(hipGetLastError());
        t_end(1);
    }
    VS_HIP(hipMemcpyAsync(h_states, states, sizeof(PairState) * n_pairs, hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    return VS_OK;
}

void vs_aligner::convert_results() {
    for (int q = 0; q < ck.fr.n_pairs(); q++) {
        const int i = ck.fr.pair_frame[q];
        vs_align_info& inf = ck.infos[i];
        tm.gn_iterations += convert_result(h_states[q], ck.fr.g(i), *this, &inf, &ck.out[i], &ck.status[i]);
        if (ck.p.phase_correlate) { inf.phase_dx = h_pres[q].dx; inf.phase_dy = h_pres[q].dy; inf.phase_response = h_pres[q].response; }
    }
}

int vs_aligner::chunk_end() {
    if (!ck.open) return set_error(VS_ERR_ARG, "no chunk in flight on this handle");
    ck.open = false;
    const int n_pairs = ck.fr.n_pairs();
    if (n_pairs > 0) {
        bool redo = ck.plan.use_host;
        if (!redo) {
            VS_TRY(wait_solver());
            for (int q = 0; q < n_pairs; q++)
                if (h_states[q].fail_reason >= 100) redo = true;   // 100: libstdc++ would have heap-selected; 101: a helper workgroup timed out -- redo on the host
            if (redo) {   // the pairs start over for host_redo
                reset_states(n_pairs);
                if (ck.plan.direct) VS_HIP(hipMemcpyAsync(descs, h_descs, sizeof(PairDesc) * n_pairs, hipMemcpyHostToDevice, stream));
                VS_HIP(hipMemcpyAsync(states, h_states, sizeof(PairState) * n_pairs, hipMemcpyHostToDevice, stream));
                if (ck.p.phase_correlate) VS_TRY(launch_phase_apply());
                VS_HIP(hipStreamSynchronize(stream));
            }
        }
        if (redo) VS_TRY(host_redo());
        convert_results();
    } else {
        VS_HIP(hipStreamSynchronize(stream));
    }
    if (timing) { t_collect(); tm.frames += ck.n; }
    seq = ck.fr.seq0 + ck.n;
    last_n = ck.n;
    return VS_OK;
}

// Kernel-level form of the keep-best-fraction step (alignment.cpp:435-492) for n_arrays independent
// warpdiff tables: out_idx[a*tx*ty + 0..count) = tile_y*tx+tile_x of the survivors in std::nth_element's order.
static int select_smallest_impl(const uint16_t* warpdiff, int n_arrays, int tx, int ty, float fraction, int32_t* out_idx,
                                int32_t* status, int mem, void* stream, int rule) {
    VS_ARG(warpdiff && out_idx && (status || rule) && n_arrays >= 1 && tx >= 1 && ty >= 1 && fraction > 0.0f && fraction <= 1.0f);
    const int nt = tx * ty;
    if (nt > kSelectCap) return set_error(VS_ERR_UNSUPPORTED, "%d tiles exceed the on-device selection capacity %d", nt, kSelectCap);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const int nsel = (int)static_cast<size_t>((size_t)nt * fraction);
    vsi::Staged a, o, st;
    VS_TRY(a.in(warpdiff, (size_t)n_arrays * nt * 2, mem, s));
    VS_TRY(o.out(out_idx, (size_t)n_arrays * nt * 4, mem));
    if (status) VS_TRY(st.out(status, (size_t)n_arrays * 4, mem));
    // (a | posR; the wave-level rounds use the first 128 bytes of posR as scratch whatever the array length)
    const size_t dyn = std::max<size_t>((((size_t)nt * 6 + 15) & ~(size_t)15), (((size_t)nt * 4 + 128 + 15) & ~(size_t)15));
    const int build = wg_build(nt);
    int device = 0;
    VS_HIP(hipGetDevice(&device));
    VS_TRY(raise_dyn_lds((const void*)kSelectBuilds[build], kDynSelect + build, device, dyn));
    hipLaunchKernelGGL(kSelectBuilds[build], dim3(n_arrays), dim3(kBuildThreads[build]), dyn, s, a.as<uint16_t>(), nt,
                       nsel, o.as<int32_t>(), status ? st.as<int32_t>() : (int32_t*)nullptr, rule);
    VS_HIP(hipGetLastError());
    if (status) VS_TRY(vsi::finish_outputs(mem, s, {&o, &st}));
    else VS_TRY(vsi::finish_outputs(mem, s, {&o}));
    return nsel;
}

extern "C" {

int vs_select_smallest(const uint16_t* warpdiff, int n_arrays, int tx, int ty, float fraction, int32_t* out_idx,
                       int32_t* status, int mem, void* stream) try {
    VS_ARG(status);
    return select_smallest_impl(warpdiff, n_arrays, tx, ty, fraction, out_idx, status, mem, stream, 0);
} VS_CATCH_ALL
// ... under VS_SELECT_STABLE's rule: smallest by (abs_delta, tile index), the survivors in ascending tile order
int vs_select_smallest_stable(const uint16_t* warpdiff, int n_arrays, int tx, int ty, float fraction, int32_t* out_idx, int mem,
                              void* stream) try {
    return select_smallest_impl(warpdiff, n_arrays, tx, ty, fraction, out_idx, nullptr, mem, stream, 1);
} VS_CATCH_ALL

vs_aligner* vs_aligner_create(const vs_aligner_params* params, int device) try {
    if (!vsi::device_ready()) return nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        set_error(VS_ERR_ARG, "device %d out of range (%d devices)", device, n);
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) { set_error(VS_ERR_HIP, "hipSetDevice(%d) failed", device); return nullptr; }
    vs_aligner* a = new vs_aligner();
    a->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
            if (prop.multiProcessorCount > 0) a->cu_count = prop.multiProcessorCount;
            a->coop_ok = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
        }
    }
    if (params) a->params = *params; else vs_aligner_params_default(&a->params);
    {   // VS_SELECT_MODE=0|1|2 (read once): the selection mode new handles start in -- for callers that cannot reach
        // vs_aligner_set_select_mode (the facade classes, the harness programs); an explicit set_select_mode still wins
        static const int env_mode = []() {
            const char* e = getenv("VS_SELECT_MODE");
            const int m = e ? atoi(e) : -1;
            if (m == VS_SELECT_STL_HOST || m == VS_SELECT_DEVICE || m == VS_SELECT_STABLE) {
                fprintf(stderr, "libvs_amd: VS_SELECT_MODE=%d -- new aligner / stabilizer handles start in selection mode %d (%s)\n", m, m,
                        m == VS_SELECT_STABLE ? "VS_SELECT_STABLE" : (m == VS_SELECT_DEVICE ? "VS_SELECT_DEVICE" : "VS_SELECT_STL_HOST"));
                return m;
            }
            return -1;
        }();
        if (env_mode >= 0) a->select_mode = env_mode;
    }
    const hipError_t se = hipStreamCreateWithFlags(&a->stream, hipStreamNonBlocking);
    if (se != hipSuccess) {
        set_error(VS_ERR_HIP, "hipStreamCreate failed");
        delete a;
        return nullptr;
    }
    return a;
} VS_CATCH_ALL_NULL

void vs_aligner_destroy(vs_aligner* a) {
    if (!a) return;
    (void)hipSetDevice(a->device);
    delete a;
}

int vs_aligner_set_select_mode(vs_aligner* a, int mode) try {
    VS_ARG(a && (mode == VS_SELECT_STL_HOST || mode == VS_SELECT_DEVICE || mode == VS_SELECT_STABLE));
    a->select_mode = mode;
    return VS_OK;
} VS_CATCH_ALL

int vs_aligner_get_select_mode(const vs_aligner* a) try {
    VS_ARG(a);
    return a->select_mode;
} VS_CATCH_ALL

int vs_aligner_set_batch_mode(vs_aligner* a, int mode) try {
    VS_ARG(a && (mode == VS_BATCH_EXCLUSIVE || mode == VS_BATCH_SHARED));
    a->batch_mode = mode;
    return VS_OK;
} VS_CATCH_ALL

int vs_aligner_reset(vs_aligner* a) try {
    VS_ARG(a);
    a->seq = 0;
    return VS_OK;
} VS_CATCH_ALL

void* vs_aligner_stream(const vs_aligner* a) { return a ? (void*)a->stream : nullptr; }

// Everything enqueued on `producer_stream` so far happens before anything the handle enqueues from now on.
int vs_aligner_wait_stream(vs_aligner* a, void* producer_stream) try {
    VS_ARG(a);
    VS_HIP(hipSetDevice(a->device));
    hipEvent_t ev = nullptr;
    VS_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, (hipStream_t)producer_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(a->stream, ev, 0);
    (void)hipEventDestroy(ev);        // the wait already holds what it needs; destruction is deferred by the runtime
    VS_HIP(e);
    return VS_OK;
} VS_CATCH_ALL

}  // extern "C"

// One align call: strides in elements of esz bytes.
struct AlignCall {
    const void* frames; size_t frame_stride; int n, stride, mem; size_t esz;
    const vs_aligner_params& p;
    vs_transform* out; int32_t* status;
};

// Host-resident frames, more than one upload's worth: pipelined ingest.  The batch is cut into chunks of host_chunk frames (about
// vsi::ingest_chunk_bytes()); an uploader thread copies chunk c+1 into the other upload area (its own stream) while chunk c runs through
// the pipeline from device memory.  Same chunks, same arithmetic as the device-resident path: results are identical.
static int align_host_pipelined(vs_aligner* a, const AlignCall& c, int host_chunk, size_t step_bytes, size_t frame_bytes) {
    const int n = c.n;
    VS_HIP(vsi::grow(a->ingest, &a->ingest_bytes, (size_t)(host_chunk - 1) * step_bytes + frame_bytes, nullptr, false, 2));
    if (!a->copy_stream) VS_HIP(hipStreamCreateWithFlags(&a->copy_stream, hipStreamNonBlocking));
    auto upload = [a, frames = c.frames, step_bytes, frame_bytes, n, host_chunk](int k) -> hipError_t {
        const int off = chunk_span(n, host_chunk, k).off, m = chunk_span(n, host_chunk, k).len;
        hipError_t e = hipSetDevice(a->device);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(a->ingest[k & 1], (const uint8_t*)frames + (size_t)off * step_bytes, (size_t)(m - 1) * step_bytes + frame_bytes,
                           hipMemcpyHostToDevice, a->copy_stream);
        return e != hipSuccess ? e : hipStreamSynchronize(a->copy_stream);
    };
    const int n_chunks = chunk_count(n, host_chunk);
    std::future<hipError_t> next = run_async(upload, 0);
    for (int k = 0; k < n_chunks; k++) {
        const int off = chunk_span(n, host_chunk, k).off, m = chunk_span(n, host_chunk, k).len;
        const hipError_t ue = next.get();                 // chunk k is in ingest[k & 1]
        if (k + 1 < n_chunks) next = run_async(upload, k + 1);   // chunk k-1 (same area) has been consumed
        int r = ue == hipSuccess ? VS_OK : set_error(VS_ERR_HIP, "frame upload failed: %s", hipGetErrorString(ue));
        if (r == VS_OK) r = a->ensure_capacity(m);
        if (r == VS_OK) r = a->run_chunk(a->ingest[k & 1], c.frame_stride, m, c.stride, VS_MEM_DEVICE, c.p, c.out + off, c.status + off, a->info.data() + off);
        if (r != VS_OK) { if (next.valid()) (void)next.get(); return r; }
    }
    return VS_OK;
}

// A device-resident batch that fits one chunk is only enqueued; align_finish completes it.
static int align_async_chunk(vs_aligner* a, const AlignCall& c) {
    VS_TRY(a->ensure_capacity(c.n));
    VS_TRY(a->chunk_begin(c.frames, c.frame_stride, c.n, c.stride, c.mem, c.p, c.out, c.status, a->info.data()));
    a->started = true; a->started_n = c.n; a->started_status = c.status;
    return VS_OK;
}

// Chunk after chunk, each completed before the next begins.
static int align_chunk_loop(vs_aligner* a, const AlignCall& c, int max_chunk) {
    for (int k = 0; k < chunk_count(c.n, max_chunk); k++) {
        const int off = chunk_span(c.n, max_chunk, k).off, m = chunk_span(c.n, max_chunk, k).len;
        VS_TRY(a->ensure_capacity(m));
        const uint8_t* base = (const uint8_t*)c.frames + (size_t)off * c.frame_stride * c.esz;
        VS_TRY(a->run_chunk(base, c.frame_stride, m, c.stride, c.mem, c.p, c.out + off, c.status + off, a->info.data() + off));
    }
    return VS_OK;
}

// First half of vs_aligner_align_batch (clip_frames == 0) / vs_aligner_align_clips (clip_frames > 0).  With `async`, a
// device-resident batch that fits one chunk is only enqueued (vs_aligner::chunk_begin) and align_finish completes it: the caller
// may do unrelated host work in between, but nothing on this handle.  Every other case completes here and align_finish just
// hands out the result.
static int align_start_impl(vs_aligner* a, const void* frames, size_t frame_stride, int n, int w, int h, int stride, int format, int mem,
                            const vs_aligner_params* params, vs_transform* out, int32_t* status, bool async) {
    VS_ARG(a && frames && out && status && n >= 1 && w >= 8 && h >= 8);
    VS_ARG(w <= 65535 && h <= 65535);                      // (tile coordinates are 16-bit; keeps w * ch and the frame spans below inside their types)
    VS_ARG(vs_format_bits(format) != 0);
    const int ch = format == VS_FMT_GRAY8 ? 1 : 3;
    VS_ARG(stride >= w * ch);
    VS_ARG(n == 1 || frame_stride >= (size_t)(h - 1) * stride + (size_t)w * ch);
    const vs_aligner_params& p = params ? *params : a->params;
    VS_ARG(p.max_iters >= 1 && p.smallest_fraction > 0.0f && p.smallest_fraction <= 1.0f);
    VS_HIP(hipSetDevice(a->device));
    if (a->W != w || a->H != h || a->fmt != format) VS_TRY(a->configure(w, h, format, p));   // alignment.cpp:155
    a->set_fraction(p.smallest_fraction);
    a->info.assign(n, vs_align_info{});
    const AlignCall c{frames, frame_stride, n, stride, mem, (size_t)(vs_format_bits(format) > 8 ? 2 : 1), p, out, status};
    int max_chunk = 0;
    VS_TRY(max_chunk_frames(a->pyr_frame, a->clip_len, &max_chunk));
    const size_t frame_bytes = ((size_t)(h - 1) * stride + (size_t)w * ch) * c.esz;
    const size_t step_bytes = n > 1 ? frame_stride * c.esz : frame_bytes;
    const int host_chunk = host_chunk_frames(max_chunk, vsi::ingest_chunk_bytes(), step_bytes, a->clip_len);
    if (mem == VS_MEM_HOST && n > host_chunk) VS_TRY(align_host_pipelined(a, c, host_chunk, step_bytes, frame_bytes));
    else if (async && mem == VS_MEM_DEVICE && n <= max_chunk) return align_async_chunk(a, c);
    else VS_TRY(align_chunk_loop(a, c, max_chunk));
    int aligned = 0;
    for (int i = 0; i < n; i++) aligned += status[i];
    a->started_result = aligned;
    return VS_OK;
}
static void align_close_clips(vs_aligner* a) {
    if (a->started_clips) { a->started_clips = false; a->clip_len = 0; a->seq = 0; }
}
// An align call that returns an error (a refused allocation, a HIP failure) ends the running sequence: the next frame is the
// first frame of a new one, exactly as a fresh handle would treat it -- the reference's protocol for a failed kernel call
// (alignment.cpp:357-367: LastWidth = -1, so the next AlignNextFrame re-initialises).  Device buffers stay as they are.
static void align_failed(vs_aligner* a) {
    a->seq = 0;
    (void)hipStreamSynchronize(a->stream);                 // nothing of the failed call is still running when its events go back to the pool
    a->ck.open = false;
    for (vs_aligner::Span& sp : a->spans) { a->event_pool.push_back(sp.a); a->event_pool.push_back(sp.b); }
    a->spans.clear();
}
int vsi::align_start(vs_aligner* a, const void* frames, size_t frame_stride, int n, int clip_frames, int w, int h, int stride, int format,
                       int mem, const vs_aligner_params* params, vs_transform* out, int32_t* status, bool async) {
    VS_ARG(a && clip_frames >= 0);
    if (a->started || a->ck.open) return set_error(VS_ERR_ARG, "an alignment is already in flight on this handle");
    a->started_result = 0;
    if (clip_frames > 0) { a->seq = 0; a->clip_len = clip_frames; a->started_clips = true; }
    // (guarded: an exception -- a host allocation that fails -- ends the call like any other stage failure, under the protocol below)
    const int r = vsi::guarded([&] { return align_start_impl(a, frames, frame_stride, n, w, h, stride, format, mem, params, out, status, async); });
    // a call REJECTED for its arguments (VS_ERR_ARG: every such test precedes the first touch of the handle's state) leaves the running
    // sequence alone -- the reference resets only when a kernel stage fails (alignment.cpp:357-367); any later error ends it
    if (r < 0) { a->started = false; align_close_clips(a); if (r != VS_ERR_ARG) align_failed(a); }
    return r;
}
int vsi::align_finish(vs_aligner* a) {
    int r = a->started_result;
    if (a->started) {
        a->started = false;
        r = vsi::guarded([&] { return a->chunk_end(); });
        if (r == VS_OK) for (int i = 0; i < a->started_n; i++) r += a->started_status[i];
    }
    align_close_clips(a);
    if (r < 0) align_failed(a);
    return r;
}
// an alignment that was started and will not be finished (an error elsewhere): drain the stream, forget the chunk
void vsi::align_abandon(vs_aligner* a) {
    if (a->ck.open) { (void)hipStreamSynchronize(a->stream); a->ck.open = false; }
    a->started = false;
    align_close_clips(a);
}

extern "C" {

int vs_aligner_align_batch(vs_aligner* a, const void* frames, size_t frame_stride, int n, int w, int h, int stride,
                           int format, int mem, const vs_aligner_params* params, vs_transform* out, int32_t* status) try {
    const int r = align_start(a, frames, frame_stride, n, 0, w, h, stride, format, mem, params, out, status, false);
    return r < 0 ? r : align_finish(a);
} VS_CATCH_ALL

// n_clips independent clips of frames_per_clip frames each, back to back in memory: the results of aligning every
// clip with its own fresh VideoAligner, computed together (every stage is one launch over all clips, so short
// clips still fill the GPU).  The handle's running sequence is reset before and after.
int vs_aligner_align_clips(vs_aligner* a, const void* frames, size_t frame_stride, int n_clips, int frames_per_clip, int w,
                           int h, int stride, int format, int mem, const vs_aligner_params* params, vs_transform* out,
                           int32_t* status) try {
    VS_ARG(a && n_clips >= 1 && frames_per_clip >= 1 && (long long)n_clips * frames_per_clip <= 0x7fffffff);
    const int r = align_start(a, frames, frame_stride, n_clips * frames_per_clip, frames_per_clip, w, h, stride, format, mem, params, out,
                              status, false);
    return r < 0 ? r : align_finish(a);
} VS_CATCH_ALL

int vs_aligner_align_next(vs_aligner* a, const void* frame, int w, int h, int stride, int format, int mem,
                          const vs_aligner_params* params, vs_transform* out) try {
    int32_t st = 0;
    int r = vs_aligner_align_batch(a, frame, 0, 1, w, h, stride, format, mem, params, out, &st);
    if (r < 0) return r;
    return st;
} VS_CATCH_ALL

int vs_aligner_enable_timing(vs_aligner* a, int enable) try {
    VS_ARG(a);
    a->timing = enable != 0;
    memset(&a->tm, 0, sizeof(a->tm));
    return VS_OK;
} VS_CATCH_ALL

int vs_aligner_get_timings(vs_aligner* a, vs_stage_timings* out) try {
    VS_ARG(a && out);
    *out = a->tm;
    return VS_OK;
} VS_CATCH_ALL

int vs_aligner_get_info(const vs_aligner* a, int i, vs_align_info* info) try {
    VS_ARG(a && info && i >= 0 && i < (int)a->info.size());
    *info = a->info[i];
    return VS_OK;
} VS_CATCH_ALL

int vs_aligner_level_dims(const vs_aligner* a, int level, int* w, int* h, int* tx, int* ty, int* ts) try {
    VS_ARG(a && level >= 0 && level < a->levels);
    const LevelDims& l = a->L[level];
    if (w) *w = l.w; if (h) *h = l.h; if (tx) *tx = l.tx; if (ty) *ty = l.ty; if (ts) *ts = l.ts;
    return VS_OK;
} VS_CATCH_ALL

// frame i of the most recent chunk lives in slot i+1 (only valid for calls that fit one chunk)
int vs_aligner_read_level_image(const vs_aligner* a, int i, int level, uint8_t* out) try {
    VS_ARG(a && out && level >= 0 && level < a->levels && i >= 0 && i < a->last_n);
    const LevelDims& l = a->L[level];
    VS_HIP(hipSetDevice(a->device));
    VS_HIP(hipMemcpy(out, a->pyr + (size_t)(i + 1) * a->pyr_frame + l.img_off, (size_t)l.w * l.h, hipMemcpyDeviceToHost));
    return VS_OK;
} VS_CATCH_ALL
int vs_aligner_read_level_argmax(const vs_aligner* a, int i, int level, int set, uint16_t* out) try {
    VS_ARG(a && out && level >= 0 && level < a->levels && i >= 0 && i < a->last_n && (set == 0 || set == 1));
    const LevelDims& l = a->L[level];
    VS_HIP(hipSetDevice(a->device));
    // the table holds {x, y} pairs per tile; the API hands out the reference's planar form (x[nt] then y[nt])
    std::vector<uint16_t> pairs((size_t)l.nt * 2);
    VS_HIP(hipMemcpy(pairs.data(), a->lm + (size_t)(i + 1) * a->lm_frame + l.lm_off + (size_t)set * 2 * l.nt, (size_t)l.nt * 4,
                     hipMemcpyDeviceToHost));
    for (int t = 0; t < l.nt; t++) { out[t] = pairs[2 * (size_t)t]; out[(size_t)l.nt + t] = pairs[2 * (size_t)t + 1]; }
    return VS_OK;
} VS_CATCH_ALL
int vs_aligner_read_level_jacobian(const vs_aligner* a, int i, int level, int set, float* out) try {
    VS_ARG(a && out && level >= 0 && level < a->levels && i >= 0 && i < a->last_n && (set == 0 || set == 1));
    const LevelDims& l = a->L[level];
    VS_HIP(hipSetDevice(a->device));
    // the table holds one float4 per tile; the API hands out the reference's planar form (4 planes of nt)
    std::vector<float> quads((size_t)l.nt * 4);
    VS_HIP(hipMemcpy(quads.data(), a->jac + (size_t)(i + 1) * a->jac_frame + l.jac_off + (size_t)set * 4 * l.nt, (size_t)l.nt * 16,
                     hipMemcpyDeviceToHost));
    for (int t = 0; t < l.nt; t++)
        for (int c = 0; c < 4; c++) out[(size_t)c * l.nt + t] = quads[4 * (size_t)t + c];
    return VS_OK;
} VS_CATCH_ALL

}  // extern "C"

// the stabilizer's side door (vs_engine.hpp)
int vsi::aligner_device(const vs_aligner* a) { return a->device; }
int vsi::aligner_batch_mode(const vs_aligner* a) { return a->batch_mode; }
void vsi::aligner_set_batch_mode(vs_aligner* a, int mode) { a->batch_mode = mode; }
