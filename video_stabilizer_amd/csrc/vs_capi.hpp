// vs_capi.hpp -- what the files of the kernel-level C ABI layer share: the argument macros, the plan (vs_call_plan.hpp), the span rings of
// vs_runtime.hip as the entry points see them, and the look-ahead passes' shared path.  Included by vs_runtime.hip, vs_capi.hip,
// vs_capi_warp.hip, vs_capi_lookahead.hip, vs_capi_ycbcr.hip and vs_capi_fidelity.hip only.
#pragma once

#include "vs_internal.hpp"
#include "vs_kernels.hpp"
#define VS_CALL_PLAN_UNIT
#include "vs_call_plan.hpp"

#include <cstring>
#include <deque>
#include <mutex>
#include <vector>

#define VS_TRY(expr) do { int _r = (expr); if (_r != VS_OK) return _r; } while (0)
#define VS_ARG(cond) do { if (!(cond)) return vsi::set_error(VS_ERR_ARG, "bad argument: %s (%s)", #cond, __func__); } while (0)
// (inside a helper or a lambda: reported under the name of the function it checks for)
#define VS_ARG_AS(cond, func) do { if (!(cond)) return vsi::set_error(VS_ERR_ARG, "bad argument: %s (%s)", #cond, func); } while (0)
// every image extent an entry point takes: positive and at most 65535 a side (tile coordinates are 16-bit, row offsets are 24-bit multiplies, and
// the products w * channels / roi.x + roi.w of the checks that follow stay inside int)
#define VS_DIMS(w, h) VS_ARG((w) > 0 && (h) > 0 && (w) <= 65535 && (h) <= 65535)

namespace vsi {

int test_fail_alloc(int k);   // vs_test_fail_alloc (include/vs_amd.h): arms the k-th allocation from now, returns the count since the last call

// ---- the span rings (vs_runtime.hip) ---------------------------------------------------------------------------------------------
// Span bookkeeping of a ring of `slots` units: reserve() hands out the next free span (plan::ring_place; every in-flight span it overlaps
// waited for and retired), commit() marks it busy behind an event on the stream, fence_span() moves that event behind the consuming kernel.
// A span is reused only after its event has completed -- also when the call fails between the take and the fence.
struct SpanRing {
    size_t slots = 0;
    size_t head = 0;
    struct Busy { size_t begin, end; hipEvent_t ev; hipStream_t stream; };
    std::deque<Busy> busy;
    std::mutex mu;                               // the owning thread (reserve / commit / fence) against vsi::retire_stream from any thread
    std::vector<hipEvent_t> pool;
    int take_event(hipEvent_t* ev);
    int retire(std::deque<Busy>::iterator it);
    int reserve(size_t n, size_t* b);            // (mu held)
    int commit(size_t b, size_t n, hipStream_t s, hipError_t enqueue_result);   // (mu held)
    int fence_span(size_t b, hipStream_t s);
    hipError_t forget_stream(hipStream_t s);
};
// A ring of T in device memory, with a pinned host mirror once something is uploaded through it.  One per (running thread, device): calls from
// different threads or for different devices never wait on each other.  take(): n units of the device half only -- the caller fills them with
// a kernel on `s`; upload(): src -> the mirror -> the same span of the device half, copy enqueued on `s`.  Either way the caller fence()s the
// span behind the kernel that reads it.
template <typename T>
struct Ring : SpanRing {
    T* host = nullptr;
    T* dev = nullptr;
    const char* too_large;                       // the message of a take beyond half the ring (one %zu)
    Ring(size_t slots_, const char* too_large_) : too_large(too_large_) { slots = slots_; }
    int take(size_t n, hipStream_t s, T** out);
    int upload(const T* src, size_t n, hipStream_t s, T** out);
    int fence(T* p, hipStream_t s) { return fence_span((size_t)(p - dev), s); }
private:
    template <typename Enqueue> int span(size_t n, bool mirrored, hipStream_t s, T** out, Enqueue enqueue);
};
// small parameter blocks (per-frame kernel parameters, matrices, candidate entries), in float4 slots
struct ParamRing : Ring<float4> {
    static constexpr size_t kSlots = plan::kParamSlots;
    ParamRing() : Ring(kSlots, "parameter block of %zu frames is too large") {}
};
// device-only scratch for per-launch coordinate tables (the table kernel writes them, the warp kernel of the same call reads them)
struct TableRing : Ring<int> {
    static constexpr size_t kInts = plan::kTableInts;
    TableRing() : Ring(kInts, "coordinate tables of %zu ints are too large") {}
};
ParamRing* param_ring();   // the calling thread's, for the current device; null without a current device of index < 16
TableRing* table_ring();
// `slots` float4 at `src` reach the parameter ring's device half on `s`: up to 128 by value (kernel arguments of vs_k_param_block, into a span
// taken from the ring), more as one upload.  *dev: the span; the caller fence()s it behind the kernel that reads it.
int send_slots(ParamRing* ring, const void* src, size_t slots, hipStream_t s, float4** dev);

// ---- a batch of frames, wherever the caller said ---------------------------------------------------------------------------------
inline int stage_in(Staged& a, const plan::Batch& b, int mem, hipStream_t s) { return a.in(b.p, b.bytes(), mem, s); }
// an output in the batch's layout, elements of esz bytes (the warp's float form: not the batch's own)
inline int stage_out(Staged& o, const plan::Batch& b, int mem, size_t esz) {
    return o.out_image(const_cast<void*>(b.p), (size_t)b.w * b.channels * esz, (size_t)b.h, (size_t)b.stride * esz, (size_t)b.n, b.fs * esz, mem);
}

// ---- the look-ahead passes' shared path: border fill, deblur, denoise, exposure statistics, coverage -----
// what every BGR-only entry point asks of its format
inline int bgr_format_ok(int format) {
    VS_ARG(format != VS_FMT_GRAY8 && vs_format_bits(format) != 0);
    return VS_OK;
}
// what the passes built on cv::warpAffine's coordinates ask of their lists and frames; pass, why: the message
constexpr char kCvShort[] = " (cv::warpAffine saturates source coordinates to short beyond)", kAsTheFill[] = ", as the border fill";
inline int lookahead_args_ok(const char* pass, const char* why, int w, int h, int n_cand) {
    VS_ARG(n_cand >= 1 && n_cand <= 16);
    if (w > 32767 || h > 32767) return set_error(VS_ERR_UNSUPPORTED, "%s: frames up to 32767 x 32767%s", pass, why);
    return VS_OK;
}

// Output frames [first, first + n) of a pass, per_call at a time (what the pass lets into half the ring).  A group's entries (Cand: vsk::FillCand or
// vsk::DeblurCand, four slots each, n_cand per frame, zeroed): entry 0 is the pass's own -- target(entry, o), which may refuse the frame;
// candidates c = 1 .. get the inverse matrix of cand_t[o * n_cand + c] and the frame pointer until the list ends, at a null frame or where
// side(entry, o * n_cand + c), which fills the entry's side word, says so.  Then on `s`, in this order: the entries' span (send_slots), with_ratios a
// device-only span of a float per entry, launch(entries on the device, ratios, first frame, frames), the fences.  A group without a single
// candidate is sent and launched only with launch_empty.  ents: scratch, the caller's so that it outlives the groups.
template <typename Cand, typename Target, typename Side, typename Launch>
int cand_groups(ParamRing* ring, int first, int n, int per_call, int n_cand, const void* const* cand_src, const vs_transform* cand_t, int w, int h,
                bool with_ratios, bool launch_empty, hipStream_t s, std::vector<Cand>& ents, Target target, Side side, Launch launch) {
    static_assert(sizeof(Cand) == 4 * sizeof(float4), "a candidate entry is four ring slots");
    for (int f0 = first; f0 < first + n; f0 += per_call) {
        const int nf = std::min(per_call, first + n - f0);
        ents.assign((size_t)nf * n_cand, Cand{});
        bool any = false;
        for (int i = 0; i < nf; i++) {
            Cand* row = &ents[(size_t)i * n_cand];
            const size_t base = (size_t)(f0 + i) * n_cand;
            VS_TRY(target(row[0], f0 + i));
            for (int c = 1; c < n_cand && cand_src[base + c] && side(row[c], base + c); c++) {
                vs_cv_inverse_matrix(&cand_t[base + c], w, h, row[c].m);
                row[c].src = cand_src[base + c];
                any = true;
            }
        }
        if (!any && !launch_empty) continue;
        float4 *cdev = nullptr, *rdev = nullptr;
        VS_TRY(send_slots(ring, ents.data(), ents.size() * 4, s, &cdev));
        if (with_ratios) VS_TRY(ring->take((ents.size() + 3) / 4, s, &rdev));
        VS_TRY(launch((Cand*)cdev, (float*)rdev, f0, nf));
        VS_TRY(ring->fence(cdev, s));
        if (rdev) VS_TRY(ring->fence(rdev, s));
    }
    return VS_OK;
}

}  // namespace vsi
