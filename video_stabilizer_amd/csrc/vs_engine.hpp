// vs_engine.hpp -- what the stabilizer (vs_stabilizer.hip) needs from the aligner (vs_engine.hip) beyond the public API.  vs_aligner stays opaque:
// its stream and select mode come through vs_aligner_stream / vs_aligner_get_select_mode.
#pragma once

#include "vs_internal.hpp"

#include <cstdlib>
#include <future>

#define VS_TRY(expr) do { int _r = (expr); if (_r < 0) return _r; } while (0)
#define VS_ARG(cond) do { if (!(cond)) return vsi::set_error(VS_ERR_ARG, "bad argument: %s (%s)", #cond, __func__); } while (0)

namespace vsi {

// host-resident video is uploaded in chunks of about this many bytes (192 MB = ~3.4 ms on PCIe 5 x16; measured on MI355X:
// 24 / 48 / 96 / 192 MB chunks reach 0.70 / 0.80 / 0.90 / 0.91 of the pinned-copy rate on a 1.5 GB batch -- every chunk
// costs a thread hand-over and a pipeline drain);
// VS_INGEST_CHUNK_BYTES overrides it (the tests use it to run many small chunks through the pipeline)
inline size_t ingest_chunk_bytes() {
    const char* e = getenv("VS_INGEST_CHUNK_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : (size_t)192 << 20;
}

// Runs `fn(args...)` on a worker thread.  std::async may throw (std::system_error) when no thread can be started; no exception
// may cross the C ABI, so in that case the task runs on the calling thread (std::launch::deferred) -- no overlap, same result.
template <typename F, typename... A>
inline std::future<hipError_t> run_async(F&& fn, A&&... args) {
    try {
        return std::async(std::launch::async, fn, args...);
    } catch (...) {
        return std::async(std::launch::deferred, fn, args...);
    }
}

// vs_aligner_align_batch (clip_frames == 0) / vs_aligner_align_clips (clip_frames > 0) in two halves (vs_engine.hip): with `async`, a
// device-resident batch that fits one chunk is only enqueued and align_finish completes it; align_abandon: started, never to be finished
int align_start(vs_aligner* a, const void* frames, size_t frame_stride, int n, int clip_frames, int w, int h, int stride, int format, int mem,
                const vs_aligner_params* params, vs_transform* out, int32_t* status, bool async);
int align_finish(vs_aligner* a);
void align_abandon(vs_aligner* a);

int aligner_device(const vs_aligner* a);
int aligner_batch_mode(const vs_aligner* a);
void aligner_set_batch_mode(vs_aligner* a, int mode);

}  // namespace vsi
