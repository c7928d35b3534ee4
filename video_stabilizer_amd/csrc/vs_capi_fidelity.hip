// vs_capi_fidelity.hip -- the fidelity statistics of the C ABI (include/vs_amd.h: vs_bgr_fidelity_batch; the rule and the kernel: vs_fidelity.hip;
// the scores, on the host: vs_host.cpp).  Two batches of images, index pairs into them; the pairs' image pointers travel through the parameter
// ring, one slot a pair, in groups of half the ring.
#include "vs_capi.hpp"
#include "vs_launch.hpp"

using namespace vsi;

extern "C" {

int vs_bgr_fidelity_batch(const void* a, size_t a_fs, int n_a, int a_stride, const void* b, size_t b_fs, int n_b, int b_stride, int w, int h, int format,
                          int n_pairs, const int32_t* pair_frames, uint64_t* stats, int mem, void* stream) try {
    VS_ARG(w >= 1 && h >= 1 && w <= 32767 && h <= 32767);
    VS_TRY(bgr_format_ok(format));
    const int bits = vs_format_bits(format);
    const plan::Batch A{a, a_fs, n_a, w, h, a_stride, 3, bits}, B{b, b_fs, n_b, w, h, b_stride, 3, bits};
    VS_ARG(n_pairs >= 0 && a && b && n_a >= 1 && n_b >= 1);
    VS_ARG(A.strides_ok() && B.strides_ok());
    if (n_pairs == 0) return VS_OK;                                     // nothing to measure, nothing launched
    VS_ARG(pair_frames && stats);
    for (size_t i = 0; i < (size_t)n_pairs; i++)
        VS_ARG(pair_frames[2 * i] >= 0 && pair_frames[2 * i] < n_a && pair_frames[2 * i + 1] >= 0 && pair_frames[2 * i + 1] < n_b);
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = A.esz();
    Staged sa, sb, o;
    VS_TRY(stage_in(sa, A, mem, s));
    const bool one_batch = b == a && B.bytes() <= A.bytes();            // b's images lie inside what was staged for a: staged once
    if (!one_batch) VS_TRY(stage_in(sb, B, mem, s));
    const char* const adev = (const char*)sa.dev;
    const char* const bdev = (const char*)(one_batch ? sa.dev : sb.dev);
    VS_TRY(o.out(stats, (size_t)n_pairs * 6 * sizeof(uint64_t), mem));
    ParamRing* ring = param_ring();
    if (!ring) return set_error(VS_ERR_HIP, "no parameter ring for this device");
    const bool on_dwords = vsk::rows_on_dwords(adev, (size_t)a_stride, a_fs, n_a, esz) && vsk::rows_on_dwords(bdev, (size_t)b_stride, b_fs, n_b, esz);
    static_assert(sizeof(vsk::FidPair) == sizeof(float4), "a pair entry is one ring slot");
    const int per_call = (int)(ParamRing::kSlots / 2);
    std::vector<vsk::FidPair> ents((size_t)std::min(n_pairs, per_call));
    for (int f0 = 0; f0 < n_pairs; f0 += per_call) {
        const int nf = std::min(per_call, n_pairs - f0);
        for (int i = 0; i < nf; i++) {
            const int32_t* pf = pair_frames + 2 * (size_t)(f0 + i);
            ents[(size_t)i] = vsk::FidPair{adev + (size_t)pf[0] * a_fs * esz, bdev + (size_t)pf[1] * b_fs * esz};
        }
        float4* pdev = nullptr;
        VS_TRY(send_slots(ring, ents.data(), (size_t)nf, s, &pdev));
        VS_HIP(vsk::bgr_fidelity((const vsk::FidPair*)pdev, w, h, a_stride, b_stride, (int)esz * 8, bits - 8, vs_format_max_value(format), on_dwords,
                                 o.as<unsigned long long>() + (size_t)f0 * 6, nf, s));
        VS_TRY(ring->fence(pdev, s));
    }
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

}  // extern "C"
