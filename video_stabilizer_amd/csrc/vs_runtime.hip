// vs_runtime.hip -- what the library keeps per process and per thread behind the kernel-level C ABI: the device check, the two allocation
// functions with their test hooks, the staging pool of the VS_MEM_HOST form, and the span rings that carry small parameter blocks and
// per-launch tables to the device.  The integer rules (capacities, placement, spans) are vs_call_plan.hpp's; events, locks and every HIP call
// are here.
#include "vs_capi.hpp"

#include <atomic>
#include <new>
#include <cstdio>
#include <cstdlib>

namespace vsi {

bool device_ready() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error(VS_ERR_HIP, "no usable HIP device (%s): libvs_amd has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return false;
    }
    return true;
}

bool& warp_keeps_solver_slot() { thread_local bool v = false; return v; }

// ---- allocation + fault injection (tests/test_alloc_failure_gpu.py) -----------------------------------------------
// g_alloc_count counts the library's allocations since the last vs_test_fail_alloc call; the one that brings it to
// g_alloc_fail_at fails with hipErrorOutOfMemory (once: the count moves on).  VS_TEST_FAIL_ALLOC=k arms it from the
// environment for programs that cannot call the hook.
// The ENVIRONMENT-driven hooks (VS_TEST_FAIL_ALLOC, VS_TEST_POISON_*) are honoured only when VS_TEST_HOOKS=1 is set as well: a stray
// variable in a production environment must not make a real allocation fail or cost every allocation a memset.
const char* test_env(const char* name) {
    static const bool on = []() { const char* h = getenv("VS_TEST_HOOKS"); return h && atoi(h) == 1; }();
    return on ? getenv(name) : nullptr;
}
static std::atomic<long long> g_alloc_count{0};
static std::atomic<long long> g_alloc_fail_at{[]() { const char* e = test_env("VS_TEST_FAIL_ALLOC"); return e ? atoll(e) : 0LL; }()};
int test_fail_alloc(int k) {
    const long long seen = g_alloc_count.exchange(0);
    g_alloc_fail_at.store(k);                              // k > 0: the k-th allocation reports out-of-memory; k < 0: it throws std::bad_alloc; 0: disarmed
    return (int)std::min<long long>(seen, 0x7fffffff);
}
static bool alloc_injected_failure() {
    const long long k = ++g_alloc_count, at = g_alloc_fail_at.load(std::memory_order_relaxed);
    if (at < 0 && k == -at) throw std::bad_alloc();        // vs_test_fail_alloc(-k): a HOST allocation failing at this point of the call
    return k == at;
}
// test hook (VS_TEST_POISON_ALLOC=<byte>): every fresh device allocation and every leased staging block starts filled with that byte, so that a
// result which depends on memory the library never wrote changes with the byte (tests/test_uninitialised_memory_gpu.py); -1: off
static int poison_byte() {
    static const int poison = []() { const char* v = test_env("VS_TEST_POISON_ALLOC"); return v ? (int)strtol(v, nullptr, 0) & 255 : -1; }();
    return poison;
}
hipError_t dev_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (alloc_injected_failure()) return hipErrorOutOfMemory;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); }      // (the sticky error belongs to this call, which reports it)
    const int poison = poison_byte();
    static const int only = []() { const char* v = test_env("VS_TEST_POISON_ONLY"); return v ? atoi(v) : 0; }();      // (0: every allocation; k: the k-th only)
    static std::atomic<int> nth{0};
    const int k = ++nth;
    if (e == hipSuccess && poison >= 0 && bytes) {
        static const long long r_off = []() { const char* v = test_env("VS_TEST_POISON_OFF"); return v ? atoll(v) : 0LL; }();
        static const long long r_len = []() { const char* v = test_env("VS_TEST_POISON_LEN"); return v ? atoll(v) : -1LL; }();
        if (only == k && r_len >= 0) {                     // (debugging aid: only bytes [off, off + len) of the k-th allocation get the byte)
            e = hipMemset(*p, 0, bytes);
            if (e == hipSuccess && r_off < (long long)bytes) e = hipMemset((char*)*p + r_off, poison, (size_t)std::min<long long>(r_len, (long long)bytes - r_off));
        } else
        e = hipMemset(*p, (only == 0 || only == k) ? poison : 0, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (only == k) std::fprintf(stderr, "[poison] allocation %d: %zu bytes\n", k, bytes);
        if (e != hipSuccess) { (void)hipFree(*p); *p = nullptr; (void)hipGetLastError(); }     // the contract: *p is nullptr on failure
    }
    return e;
}
hipError_t pinned_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (alloc_injected_failure()) return hipErrorOutOfMemory;
    const hipError_t e = hipHostMalloc(p, bytes);
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); }
    return e;
}

// ---- the staging pool ------------------------------------------------------------------------------------------------------------
// Free blocks are kept per process (any thread, any device: a block remembers its device); a lease takes the smallest free block that
// is large enough, or allocates one (capacities are rounded up: plan::stage_capacity).  At most kStageKeepBlocks / kStageKeepBytes stay
// cached; what does not fit is freed on release.  Nothing is freed at process exit (the HIP runtime may already be gone).
namespace {
constexpr size_t kStageKeepBlocks = 24, kStageKeepBytes = (size_t)3 << 30;
struct StagePool {
    std::mutex mu;
    std::vector<StageBlock*> free_;
    size_t kept_bytes = 0;
};
StagePool& stage_pool() { static StagePool* p = new StagePool(); return *p; }
void stage_destroy(StageBlock* b) {
    if (b->dev) (void)hipFree(b->dev);
    if (b->pin) (void)hipHostFree(b->pin);
    delete b;
}
// the smallest free block of the device that holds cap bytes leaves the pool; null if there is none
StageBlock* stage_take_free(int device, size_t cap) {
    StagePool& p = stage_pool();
    std::lock_guard<std::mutex> g(p.mu);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < p.free_.size(); i++)
        if (p.free_[i]->device == device && p.free_[i]->cap >= cap && (best == (size_t)-1 || p.free_[i]->cap < p.free_[best]->cap)) best = i;
    if (best == (size_t)-1) return nullptr;
    StageBlock* b = p.free_[best];
    p.free_.erase(p.free_.begin() + (long)best);
    p.kept_bytes -= b->cap;
    return b;
}
thread_local unsigned long long t_sync_epoch = 1;
}  // namespace
unsigned long long host_sync_epoch() { return t_sync_epoch; }
void host_synced() { ++t_sync_epoch; }

StageBlock* stage_acquire(size_t bytes) {
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); set_error(VS_ERR_HIP, "hipGetDevice failed (staging)"); return nullptr; }
    const size_t cap = plan::stage_capacity(bytes ? bytes : 1);
    const int poison = poison_byte();
    if (StageBlock* b = stage_take_free(device, cap)) {
        // test hook: a reused block starts from the poison byte like a fresh allocation
        if (poison >= 0 && (hipMemset(b->dev, poison, b->cap) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
            (void)hipGetLastError(); stage_destroy(b); set_error(VS_ERR_HIP, "poisoning a staging block failed"); return nullptr;
        }
        if (poison >= 0) memset(b->pin, poison, b->cap);
        return b;
    }
    StageBlock* b = new StageBlock();
    b->cap = cap; b->device = device;
    hipError_t e = dev_alloc(&b->dev, cap);
    if (e == hipSuccess) e = pinned_alloc(&b->pin, cap);
    if (e != hipSuccess) {
        stage_destroy(b);
        set_error(VS_ERR_HIP, "staging block of %zu bytes: %s", cap, hipGetErrorString(e));
        return nullptr;
    }
    if (poison >= 0) memset(b->pin, poison, cap);
    return b;
}
void stage_release(StageBlock* b) {
    if (!b) return;
    {
        StagePool& p = stage_pool();
        std::lock_guard<std::mutex> g(p.mu);
        if (p.free_.size() < kStageKeepBlocks && p.kept_bytes + b->cap <= kStageKeepBytes) {
            p.free_.push_back(b);
            p.kept_bytes += b->cap;
            return;
        }
        // the cache is full: drop the smallest cached block if this one is larger (large blocks are the expensive ones to make)
        size_t small = (size_t)-1;
        for (size_t i = 0; i < p.free_.size(); i++)
            if (small == (size_t)-1 || p.free_[i]->cap < p.free_[small]->cap) small = i;
        if (small != (size_t)-1 && p.free_[small]->cap < b->cap && p.kept_bytes - p.free_[small]->cap + b->cap <= kStageKeepBytes) {
            std::swap(b, p.free_[small]);
            p.kept_bytes += p.free_[small]->cap - b->cap;
        }
    }
    stage_destroy(b);
}

Staged::~Staged() {
    if (!blk) return;
    // an error return between the first enqueue and the call's synchronisation: work that reads or writes the block may still be in flight
    if (epoch == host_sync_epoch()) { (void)hipDeviceSynchronize(); (void)hipGetLastError(); }
    stage_release(blk);
}
int Staged::lease(size_t n) {
    if (blk) { stage_release(blk); blk = nullptr; }
    blk = stage_acquire(n);
    if (!blk) return VS_ERR_HIP;
    dev = blk->dev;
    epoch = host_sync_epoch();
    return VS_OK;
}
int Staged::in(const void* ptr, size_t n, int mem, hipStream_t s) {
    bytes = n; is_out = false;
    if (mem == VS_MEM_DEVICE) { dev = const_cast<void*>(ptr); staged = false; return VS_OK; }
    staged = true; host = const_cast<void*>(ptr);
    if (int r = lease(n)) return r;
    if (n) {
        memcpy(blk->pin, ptr, n);
        VS_HIP(hipMemcpyAsync(dev, blk->pin, n, hipMemcpyHostToDevice, s));
    }
    return VS_OK;
}
int Staged::out(void* ptr, size_t n, int mem) {
    bytes = n; is_out = true;
    if (mem == VS_MEM_DEVICE) { dev = ptr; staged = false; return VS_OK; }
    staged = true; host = ptr;
    return lease(n);
}
int Staged::out_image(void* ptr, size_t row_bytes_, size_t rows_, size_t pitch_, size_t frames_, size_t frame_pitch_, int mem) {
    const int r = out(ptr, plan::out_image_bytes(row_bytes_, rows_, pitch_, frames_, frame_pitch_), mem);
    const bool dense = plan::out_image_dense(row_bytes_, rows_, pitch_, frames_, frame_pitch_);
    if (r == VS_OK && staged && !dense) { row_bytes = row_bytes_; rows = rows_; pitch = pitch_; frames = frames_; frame_pitch = frame_pitch_; }
    return r;
}
int Staged::finish(hipStream_t s) {
    if (!(staged && is_out && bytes)) return VS_OK;
    VS_HIP(hipMemcpyAsync(blk->pin, dev, bytes, hipMemcpyDeviceToHost, s));     // dense: the gaps between rows travel too and are dropped by complete()
    copied_back = true;
    return VS_OK;
}
void Staged::complete() {
    if (!copied_back) return;
    copied_back = false;
    const char* m = (const char*)blk->pin;
    if (rows == 0) { memcpy(host, m, bytes); return; }
    for (size_t f = 0; f < frames; f++)               // pitched: the bytes between the rows stay as the caller had them
        for (size_t r = 0; r < rows; r++)
            memcpy((char*)host + f * frame_pitch + r * pitch, m + f * frame_pitch + r * pitch, row_bytes);
}
int finish_outputs(int mem, hipStream_t s, std::initializer_list<Staged*> outs) {
    for (Staged* o : outs) if (int r = o->finish(s)) return r;
    if (mem != VS_MEM_HOST) return VS_OK;
    VS_HIP(hipStreamSynchronize(s));
    host_synced();
    for (Staged* o : outs) o->complete();
    return VS_OK;
}

// ---- the span rings (vs_capi.hpp) ------------------------------------------------------------------------------------------------
// Events are pooled per ring.
int SpanRing::take_event(hipEvent_t* ev) {
    if (!pool.empty()) { *ev = pool.back(); pool.pop_back(); return VS_OK; }
    VS_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return VS_OK;
}
int SpanRing::retire(std::deque<Busy>::iterator it) {
    VS_HIP(hipEventSynchronize(it->ev));
    pool.push_back(it->ev);
    busy.erase(it);
    return VS_OK;
}
// (mu held) the next span of n units: [*b, *b + n), every in-flight span that overlaps it waited for and retired
int SpanRing::reserve(size_t n, size_t* b) {
    const plan::Span sp = plan::ring_place(head, n, slots);
    head = *b = sp.begin;
    for (bool again = true; again;) {
        again = false;
        for (auto it = busy.begin(); it != busy.end(); ++it)
            if (plan::spans_overlap(sp, plan::Span{it->begin, it->end})) { VS_TRY(retire(it)); again = true; break; }
    }
    while (busy.size() > 64) VS_TRY(retire(busy.begin()));   // keep the list short: retire the oldest
    return VS_OK;
}
// (mu held) the span is busy from now on: an event recorded on `s` right behind what the caller has just enqueued
int SpanRing::commit(size_t b, size_t n, hipStream_t s, hipError_t enqueue_result) {
    Busy bz{b, b + n, nullptr, s};
    VS_TRY(take_event(&bz.ev));
    hipError_t err = enqueue_result;
    if (err == hipSuccess) err = hipEventRecord(bz.ev, s);
    if (err != hipSuccess) { pool.push_back(bz.ev); VS_HIP(err); }
    busy.push_back(bz);
    head = b + n;
    return VS_OK;
}
// called after the consuming kernel has been enqueued on `s`: the span that begins at b stays busy until that kernel is done
int SpanRing::fence_span(size_t b, hipStream_t s) {
    std::lock_guard<std::mutex> g(mu);
    for (auto& z : busy)
        if (z.begin == b) { VS_HIP(hipEventRecord(z.ev, s)); z.stream = s; return VS_OK; }
    return VS_OK;
}
// every span whose event was recorded on `s` is waited for and retired NOW, while the stream still exists: this runtime's
// hipEventSynchronize looks at the stream an event was last recorded on, so an event must never outlive that stream in here
hipError_t SpanRing::forget_stream(hipStream_t s) {
    std::lock_guard<std::mutex> g(mu);
    hipError_t first = hipSuccess;
    for (auto it = busy.begin(); it != busy.end();) {
        if (it->stream == s) {
            const hipError_t e = hipEventSynchronize(it->ev);
            if (e != hipSuccess && first == hipSuccess) first = e;
            pool.push_back(it->ev); it = busy.erase(it);
        }
        else ++it;
    }
    return first;
}

// the one body of take and upload: lock, size, the ring's memory on first use (the pinned half only for an upload), reserve, the caller's
// enqueue (span begin -> its result), commit
template <typename T> template <typename Enqueue>
int Ring<T>::span(size_t n, bool mirrored, hipStream_t s, T** out, Enqueue enqueue) {
    std::lock_guard<std::mutex> g(mu);
    if (!plan::take_fits(n, slots)) return set_error(VS_ERR_ARG, too_large, n);
    if (mirrored && !host) VS_HIP(pinned_alloc((void**)&host, slots * sizeof(T)));
    if (!dev) VS_HIP(dev_alloc((void**)&dev, slots * sizeof(T)));
    size_t b = 0;
    VS_TRY(reserve(n, &b));
    VS_TRY(commit(b, n, s, enqueue(b)));
    *out = dev + b;
    return VS_OK;
}
template <typename T> int Ring<T>::take(size_t n, hipStream_t s, T** out) {
    return span(n, false, s, out, [](size_t) { return hipSuccess; });
}
template <typename T> int Ring<T>::upload(const T* src, size_t n, hipStream_t s, T** out) {
    return span(n, true, s, out, [&](size_t b) {
        memcpy(host + b, src, n * sizeof(T));
        return hipMemcpyAsync(dev + b, host + b, n * sizeof(T), hipMemcpyHostToDevice, s);
    });
}
template struct Ring<float4>;
template struct Ring<int>;

// A thread takes a ring pair per device on first use and hands it back to a process-wide pool when it exits; the next thread that
// needs one for that device reuses it (its in-flight spans are retired by event as always).  So the pinned / device memory
// held is bounded by the largest number of threads that were inside bgr_image_warp entry points at the same time, not by the
// number of threads that ever called one (a thread-per-frame caller used to leave 1 MiB behind per thread).  Nothing is freed
// at thread or process exit: the HIP runtime may already be gone by then.
namespace {
struct Rings { ParamRing params; TableRing tables; };
struct RingPool {
    std::mutex mu;
    std::vector<Rings*> free_[16];
    std::vector<Rings*> all;                     // every ring pair ever made (rings are never destroyed)
};
RingPool& ring_pool() { static RingPool* p = new RingPool(); return *p; }      // never destroyed: outlives every thread's holder
struct RingHolder {
    Rings* r[16] = {};
    ~RingHolder() {
        RingPool& p = ring_pool();
        std::lock_guard<std::mutex> g(p.mu);
        for (int d = 0; d < 16; d++) if (r[d]) p.free_[d].push_back(r[d]);
    }
};
Rings* thread_rings() {
    thread_local RingHolder holder;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= 16) return nullptr;
    if (!holder.r[device]) {
        RingPool& p = ring_pool();
        std::lock_guard<std::mutex> g(p.mu);
        if (!p.free_[device].empty()) { holder.r[device] = p.free_[device].back(); p.free_[device].pop_back(); }
        else { holder.r[device] = new Rings(); p.all.push_back(holder.r[device]); }
    }
    return holder.r[device];
}
}  // namespace
ParamRing* param_ring() { Rings* r = thread_rings(); return r ? &r->params : nullptr; }
TableRing* table_ring() { Rings* r = thread_rings(); return r ? &r->tables : nullptr; }

// A stream is about to be destroyed (a handle's own stream: ~vs_aligner; a caller's stream: vs_stream_retire): nothing in the
// library may refer to it afterwards.
hipError_t retire_stream(hipStream_t s) {
    std::vector<Rings*> rings;
    {
        RingPool& p = ring_pool();
        std::lock_guard<std::mutex> g(p.mu);
        rings = p.all;
    }
    hipError_t first = hipSuccess;
    for (Rings* r : rings) {
        const hipError_t e1 = r->params.forget_stream(s), e2 = r->tables.forget_stream(s);
        if (e1 != hipSuccess && first == hipSuccess) first = e1;
        if (e2 != hipSuccess && first == hipSuccess) first = e2;
    }
    return first;
}

}  // namespace vsi

// Small parameter blocks (up to kParamBlockSlots float4: the per-frame parameters + extents of up to 64 frames) reach the device as KERNEL ARGUMENTS of a
// one-workgroup kernel that writes them into the ring's span: no host-to-device copy stands between the host's numbers and the warp kernel for the
// per-frame drop-in call and the small batches of the parity tests (round 6, profiles/r06_flake.md: the matrix upload was the second of the two
// runtime-ordered transfers the round-5 failure could have come from).
namespace {
constexpr int kParamBlockSlots = 128;
struct ParamBlock { float4 v[kParamBlockSlots]; };
__global__ __launch_bounds__(kParamBlockSlots) void vs_k_param_block(ParamBlock b, float4* __restrict__ dst, int n) {
    const int i = (int)threadIdx.x;
    if (i < n) dst[i] = b.v[i];
}
}  // namespace
int vsi::send_slots(ParamRing* ring, const void* src, size_t slots, hipStream_t s, float4** dev) {
    if (slots > (size_t)kParamBlockSlots) return ring->upload((const float4*)src, slots, s, dev);
    ParamBlock blk{};
    memcpy(blk.v, src, slots * sizeof(float4));
    VS_TRY(ring->take(slots, s, dev));
    hipLaunchKernelGGL(vs_k_param_block, dim3(1), dim3(kParamBlockSlots), 0, s, blk, *dev, (int)slots);
    VS_HIP(hipGetLastError());
    return VS_OK;
}
