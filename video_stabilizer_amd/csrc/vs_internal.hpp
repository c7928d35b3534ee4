// vs_internal.hpp -- shared by the translation units behind the C ABI.
#pragma once

#include "../../include/vs_amd.h"

#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <initializer_list>

namespace vsi {
// records a thread-local message for vs_last_error() and returns `code`
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// No exception crosses the C ABI (include/vs_amd.h).  caught(): inside a catch block, turns the in-flight exception into VS_ERR_NOMEM and a
// message; guarded(f): runs f() and stops whatever it throws.  Every extern "C" entry point that can allocate on the host is a
// function-try-block ending in VS_CATCH_ALL; the engine calls also guard their inner stages, so that their failure protocol runs.
int caught() noexcept;
template <typename F>
inline int guarded(F&& f) noexcept {
    try { return f(); } catch (...) { return caught(); }
}
// The vs_deblur_params the library accepts (include/vs_amd.h): with r <= min(max_ratio, 2^53) (S < 2^53) a weight is
// at most r^2 / sensitivity, so under r^2 / sensitivity <= 2^100 the sums of at most 15 weights times samples <= 65535 stay below
// 2^4 * 2^100 * 2^16 * (1 + 2^-24)^64 < 2^121: acc and W are finite for every frame.  (fp32 overflows from r^2 / sensitivity of about 2^108.)
inline bool deblur_params_finite(float sensitivity, float max_ratio) {
    if (!(sensitivity > 0.0f && sensitivity <= 3.0e38f && max_ratio > 0.0f && max_ratio <= 1.0e18f)) return false;
    const double r = (double)max_ratio < 9007199254740992.0 ? (double)max_ratio : 9007199254740992.0;
    return r * r <= (double)sensitivity * 0x1p100;
}
// The other passes' parameter ranges (include/vs_amd.h), each written once: the kernel-level entry points (vs_capi_lookahead.hip,
// vs_capi_warp.hip) and the stabilizer's setters (vs_stabilizer.hip) ask these.  What a NULL pointer means stays with the caller.
inline bool denoise_params_valid(const vs_denoise_params& p) { return p.strength >= 1 && p.strength <= 255; }
inline bool rolling_params_valid(const vs_rolling_params& p) { return p.readout >= -1.0 && p.readout <= 1.0; }   // (a NaN fails both)
inline bool deflicker_params_valid(const vs_deflicker_params& p) { return p.step >= 1 && p.step <= 64; }
inline bool scene_params_valid(const vs_scene_params& p) { return p.step >= 1 && p.step <= 64 && p.threshold >= 1 && p.threshold <= 255; }
inline bool sharpen_params_valid(const vs_sharpen_params& p) { return p.strength >= 1 && p.strength <= 32; }
inline bool fill_blend_params_valid(const vs_fill_blend_params& p) { return p.feather >= 0 && p.feather <= 6 && (p.match == 0 || p.match == 1); }
// Frames per upload of a host-resident batch, for the aligner and the stabilizer alike: about ingest_bytes (vsi::ingest_chunk_bytes()), at
// least 4, whole clips, within max_chunk.
inline int host_chunk_frames(int max_chunk, size_t ingest_bytes, size_t step_bytes, int clip_len) {
    int c = (int)std::min<size_t>((size_t)max_chunk, std::max<size_t>(4, ingest_bytes / std::max<size_t>(1, step_bytes)));
    if (clip_len > 0) c = std::max(clip_len, c - c % clip_len);
    return c;
}
// vs_lens_map with VS_MEM_HOST (vs_host.cpp; the rule: vs_lens.hpp): checks its arguments, needs no device
int lens_map_host(const vs_lens_params* p, int w, int h, int32_t* map, int map_stride);
constexpr int kSharedMinPairs = 32;   // VS_BATCH_SHARED: launches of at least this many pairs take the aligner's small-footprint solver build
}  // namespace vsi
#define VS_CATCH_ALL catch (...) { return vsi::caught(); }
#define VS_CATCH_ALL_NULL catch (...) { (void)vsi::caught(); return nullptr; }

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#define VS_HIP(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t _e = (expr);                                                                          \
        if (_e != hipSuccess)                                                                            \
            return vsi::set_error(VS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace vsi {

// Every device / pinned-host allocation of the library goes through these two, so that tests can make the k-th one fail
// (vs_test_fail_alloc, include/vs_amd.h).  On failure *p is nullptr.
hipError_t dev_alloc(void** p, size_t bytes);
hipError_t pinned_alloc(void** p, size_t bytes);
// getenv(name) for the environment-driven test hooks: null unless VS_TEST_HOOKS=1 is set as well (that gate is read once per process)
const char* test_env(const char* name);

// A scratch buffer of a handle grows to `need` bytes (`count` buffers that share one size field).  sync: work on `ws` may still read the old
// block.  The handle's fields are zeroed before the allocation: after a failed one the handle holds no buffer and the next call starts over
// (tests/test_alloc_failure_gpu.py).
inline hipError_t grow(void** buf, size_t* bytes, size_t need, hipStream_t ws = nullptr, bool sync = false, int count = 1) {
    if (*bytes >= need) return hipSuccess;
    hipError_t e = sync ? hipStreamSynchronize(ws) : hipSuccess;
    if (e != hipSuccess) return e;
    for (int k = 0; k < count; k++) { if (buf[k]) (void)hipFree(buf[k]); buf[k] = nullptr; }
    *bytes = 0;
    for (int k = 0; e == hipSuccess && k < count; k++) e = dev_alloc(&buf[k], need);
    if (e == hipSuccess) *bytes = need;
    return e;
}
// One scratch buffer of a handle and its size, under grow's protocol; drop: the handle holds no buffer again.
struct Scratch {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t grow(size_t need, hipStream_t ws = nullptr, bool sync = false) { return vsi::grow(&p, &bytes, need, ws, sync); }
    void drop() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// RAII device allocation used by the host-staged (VS_MEM_HOST) form of the kernel-level calls.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) {
        if (p) { (void)hipFree(p); p = nullptr; }
        bytes = n;
        return dev_alloc(&p, n ? n : 1);
    }
    template <typename T> T* as() const { return (T*)p; }
};

// Staging for the host-memory (VS_MEM_HOST) form of the kernel-level calls.  A block = device memory + a PINNED host mirror of the same size,
// leased from a process-wide pool (vs_runtime.hip): no hipMalloc / hipFree per call, and the HIP runtime never sees the caller's pageable memory --
// inputs are copied into the mirror by the CPU and travel as one dense pinned H2D copy; outputs come back as one dense D2H copy into the mirror
// and the CPU scatters the rows into the caller's buffer after the stream has been synchronised.  (Until round 5 outputs went back with one
// hipMemcpy2DAsync per frame straight into pageable, possibly 2-byte-aligned caller memory: profiles/r06_flake.md.)
struct StageBlock {
    void* dev = nullptr;
    void* pin = nullptr;
    size_t cap = 0;
    int device = 0;
};
StageBlock* stage_acquire(size_t bytes);                   // nullptr on failure (last error set)
void stage_release(StageBlock* b);
// "the calling thread has synchronised with every copy and kernel it enqueued on a staged block": bumped by finish_outputs() and by entry
// points that synchronise themselves; a Staged that dies without having seen it (an error return) quiesces the device before its block is reused
unsigned long long host_sync_epoch();
void host_synced();

// An argument that lives wherever the caller said (`mem`): for device memory it is the caller's
// pointer; for host memory it is a staged device copy (uploaded for inputs, downloaded for outputs).
struct Staged {
    StageBlock* blk = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    bool is_out = false, staged = false, copied_back = false;
    unsigned long long epoch = 0;
    Staged() = default;
    Staged(const Staged&) = delete;
    Staged& operator=(const Staged&) = delete;
    ~Staged();
    int in(const void* ptr, size_t n, int mem, hipStream_t s);
    int out(void* ptr, size_t n, int mem);
    // an image output: `frames` images of `rows` rows of `row_bytes` bytes, `pitch` bytes from row to row and `frame_pitch` from
    // image to image.  Only the rows' own bytes reach the caller: the padding between them may be the caller's neighbouring pixels.
    int out_image(void* ptr, size_t row_bytes, size_t rows, size_t pitch, size_t frames, size_t frame_pitch, int mem);
    int finish(hipStream_t s);   // staged outputs: ONE dense D2H into the pinned mirror (async; complete() after the stream has been synchronised)
    void complete();             // mirror -> the caller's memory (CPU; rows only for pitched images)
    size_t row_bytes = 0, rows = 0, pitch = 0, frames = 0, frame_pitch = 0;   // set by out_image (pitch != row_bytes or gaps between frames)
    template <typename T> T* as() const { return (T*)dev; }
private:
    int lease(size_t n);
};
// the tail of every kernel-level call: D2H of the staged outputs, (host memory) synchronise, rows into the caller's buffers
int finish_outputs(int mem, hipStream_t s, std::initializer_list<Staged*> outs);

// VS_WARP_BILINEAR_CV with border fill (the rule: vs_fill.hip) on device-resident frames; vs_bgr_image_warp_fill_batch is the index-based wrapper over
// it.  Output frame o = frame o of the batch at `src` warped by cand_t[o * n_cand]; its uncovered pixels come from candidates c = 1 .. n_cand-1:
// the frame at cand_src[o * n_cand + c] (any device pointer, w x h, rows of src_stride elements; null ends the list; entry c == 0 is not read)
// under cand_t[o * n_cand + c].  Host arrays; enqueue only.  blend (NULL or {0, 0}: off, the plain fill launch for launch): the blend rule's two
// switches; with match, cand_sums[o * n_cand + c] is where the three channel sums of that candidate's original frame lie in device memory.
int bgr_warp_fill_ptrs(const void* src, size_t src_fs, int n_out, int w, int h, int src_stride, int bits, int n_cand, const void* const* cand_src,
                       const vs_transform* cand_t, int border, int max_value, int roi_x, int roi_y, int roi_w, int roi_h, void* dst, size_t dst_fs,
                       int dst_stride, hipStream_t s, const uint64_t* const* cand_sums = nullptr, const vs_fill_blend_params* blend = nullptr);

// The deblur pass (the rule: vs_deblur.hip) on device-resident frames; vs_bgr_deblur_batch is the index-based wrapper over it.  Output frame o
// = the frame at cand_src[o * n_cand] blended with its candidates c = 1 .. n_cand-1: the frame at cand_src[o * n_cand + c] (any device pointer,
// w x h, rows of src_stride elements; null ends the list) under cand_t[o * n_cand + c]; cand_sharp[o * n_cand + c]: where that frame's sharpness
// lies in device memory (the kernels read it there; the host never does).  dst: full frames.  Host arrays; enqueue only.
int bgr_deblur_ptrs(int n_out, int w, int h, int src_stride, int format, int n_cand, const void* const* cand_src, const uint64_t* const* cand_sharp,
                    const vs_transform* cand_t, const vs_deblur_params* params, void* dst, size_t dst_fs, int dst_stride, hipStream_t s);

// The denoise pass (the rule: vs_denoise.hip) on device-resident frames; vs_bgr_denoise_batch is the index-based wrapper over it.  Output frame o
// = the frame at cand_src[o * n_cand] averaged with its candidates c = 1 .. n_cand-1: the frame at cand_src[o * n_cand + c] (any device pointer,
// w x h, rows of src_stride elements; null ends the list) under cand_t[o * n_cand + c].  dst: full frames.  Host arrays; enqueue only.
int bgr_denoise_ptrs(int n_out, int w, int h, int src_stride, int format, int n_cand, const void* const* cand_src, const vs_transform* cand_t,
                     const vs_denoise_params* params, void* dst, size_t dst_fs, int dst_stride, hipStream_t s);

// The rolling-shutter pass (the rule: vs_rolling.hip) on device-resident frames; vs_bgr_rolling_batch is the index-based wrapper over it.  Output
// frame o = the frame at cand_src[2 o] (any device pointer, w x h, rows of src_stride elements) corrected by the motion cand_t[2 o + 1] to the frame
// that follows it; cand_src[2 o + 1] is only compared with null (null: no motion known, the frame is copied) and never followed.  dst: full frames.
// Host arrays; enqueue only.
int bgr_rolling_ptrs(int n_out, int w, int h, int src_stride, int format, const void* const* cand_src, const vs_transform* cand_t,
                     const vs_rolling_params* params, void* dst, size_t dst_fs, int dst_stride, hipStream_t s);

// The deflicker's statistics pass (the rule: vs_deflicker.hip) on device-resident frames; vs_bgr_exposure_stats_batch is the index-based wrapper
// over it.  The pairs of output frame o: the frame at cand_src[o * n_cand] with its candidates c = 1 .. n_cand-1 (any device pointer, w x h, rows of
// src_stride elements; null ends the list) under cand_t[o * n_cand + c].  stats: n_out x n_cand x 8 words of device memory, zeroed on `s` first.
// Host arrays; enqueue only.
int exposure_stats_ptrs(int n_out, int w, int h, int src_stride, int format, int n_cand, const void* const* cand_src, const vs_transform* cand_t,
                        const vs_deflicker_params* params, uint64_t* stats, hipStream_t s);

// The scene-cut statistics (the rule: vs_scene.hip) on device-resident frames; vs_bgr_scene_stats_batch is the index-based wrapper over it.  Pair
// i: the target frame at pair_src[2 i] and the candidate frame at pair_src[2 i + 1] (any device pointers, w x h, rows of src_stride elements) under
// pair_t[i].  stats: n_pairs x 2 words of device memory, zeroed on `s` first.  Host arrays; enqueue only.
int scene_stats_ptrs(int n_pairs, int w, int h, int src_stride, int format, const void* const* pair_src, const vs_transform* pair_t,
                     const vs_scene_params* params, uint64_t* stats, hipStream_t s);

// The sharpen pass (the rule: vs_sharpen.hip) on device-resident windows; vs_bgr_sharpen_batch is the staging wrapper over it.  Image i: the
// roi_w x roi_h window at src + i * src_fs elements (rows of src_stride elements) of a w x h output frame warped under t[i]; dst likewise.  The
// two ranges must not overlap.  Host array; enqueue only.
int bgr_sharpen_ptrs(const void* src, size_t src_fs, int n, int w, int h, int format, const vs_transform* t, const vs_sharpen_params* params, int roi_x,
                     int roi_y, int roi_w, int roi_h, int src_stride, void* dst, size_t dst_fs, int dst_stride, hipStream_t s);

// The inpaint's coverage index (the rule: vs_inpaint.hip) on the device; vs_bgr_fill_coverage_batch is the index-based wrapper over it.  The
// candidates of output frame o as bgr_warp_fill_ptrs takes them -- cand_t[o * n_cand + c], a null cand_src entry ends the list, entry 0 is the
// frame itself; no frame is read.  cov: n_out indices of roi_h rows of cov_stride bytes, cov_fs bytes apart, in device memory; open_count (may
// be null): n_out words of device memory, zeroed on `s` first, then every frame's number of zeros.  fn: the function that argument errors name.
// Host arrays; enqueue only.
int fill_coverage_ptrs(int n_out, int w, int h, int n_cand, const void* const* cand_src, const vs_transform* cand_t, int roi_x, int roi_y, int roi_w,
                       int roi_h, uint8_t* cov, size_t cov_fs, int cov_stride, uint32_t* open_count, hipStream_t s, const char* fn);

bool device_ready();   // true when a HIP device is usable (sets last error otherwise)
// What vs_stabilizer_process_batch_ycbcr (vs_capi_ycbcr.hip), a wrapper around vs_stabilizer_process_batch, needs of a handle (vs_stabilizer.hip):
// the two BGR buffers the handle keeps for it -- [0] the converted input batch, [1] the inner call's outputs; grown on demand, never allocated
// unless that entry point is called, freed by vs_stabilizer_destroy -- the crop in force and the handle's device.
struct YcbcrHold { void* buf[2] = {nullptr, nullptr}; size_t bytes[2] = {0, 0}; };
YcbcrHold* stab_ycbcr_hold(vs_stabilizer* s);
int stab_crop(const vs_stabilizer* s);      // max(crop_pixels, 0)
int stab_device(const vs_stabilizer* s);
void stab_delivered_size(const vs_stabilizer* s, int w, int h, int* dw, int* dh);   // what a call with w x h frames delivers (vs_stabilizer_set_output_size)
// Set by the engine around warp launches that run beside the NEXT group's alignment (vs_stabilizer_process_batch / _clips, overlapped): the small-footprint
// solver build moves into a CU as soon as ONE warp workgroup leaves it, which needs the warp's workgroup to hold at least the solver's 35 KB of LDS -- the
// standard 31 KB window does (with the CU's slack), the COMPACT six-wave instantiation's 26 KB does not (c5: 20.3 k -> 18.4 k frames/s with it).  Thread-local:
// a handle is used by one thread at a time, and the hint must not reach another thread's calls.
bool& warp_keeps_solver_slot();
// `s` is about to be destroyed: wait for and drop everything the library still tracks on it (bgr_image_warp's parameter ring
// keeps an event per in-flight call; an event must not outlive the stream it was recorded on)
hipError_t retire_stream(hipStream_t s);   // first error of the waits (the references are dropped either way)

}  // namespace vsi
#endif
