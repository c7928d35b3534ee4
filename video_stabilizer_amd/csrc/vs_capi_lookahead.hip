// vs_capi_lookahead.hip -- the look-ahead passes of the C ABI (include/vs_amd.h) next to the border fill (vs_capi_warp.hip): channel sums,
// sharpness and deblur, denoise, rolling-shutter correction, remap and lens map, exposure statistics / gains / gain, scene-cut statistics, sharpen, coverage index and inpaint.  Each pass that takes candidate lists is a
// *_ptrs function in vsi (device-resident frames, enqueue only: the engine's form) and an index-based *_batch wrapper over it; what brings a
// list to a kernel is cand_groups (vs_capi.hpp).
#include "vs_capi.hpp"
#include "vs_lens.hpp"

#include <cstdlib>

using namespace vsi;

namespace {
// The argument rule of a pass over BGR frames with candidate lists, for its *_ptrs function and its index-based wrapper alike (fn: the one the
// caller entered): extent, format, the lists' length and -- pass != null: a pass built on cv::warpAffine's coordinates; pass, why:
// the message -- the frame limit, then the lists and outputs (ptrs: their pointers are there) and the strides; out: the output frames, null
// for a pass that writes none.
int pass_args_ok(const char* fn, const char* pass, const char* why, int w, int h, int format, int n_cand, bool ptrs, int n_out, int src_stride,
                 const plan::Batch* out) {
    VS_ARG_AS(w > 0 && h > 0 && w <= 65535 && h <= 65535, fn);
    VS_TRY(bgr_format_ok(format));
    if (pass) VS_TRY(lookahead_args_ok(pass, why, w, h, n_cand));
    VS_ARG_AS(ptrs && n_out >= 1 && n_cand >= 1 && n_cand <= 16 && src_stride >= w * 3, fn);
    VS_ARG_AS(!out || out->strides_ok(), fn);
    return VS_OK;
}
// the same for a pass over a plain batch: n frames in, and (out != null) as many out
int batch_args_ok(const char* fn, int format, bool ptrs, const plan::Batch& in, const plan::Batch* out) {
    VS_ARG_AS(in.w > 0 && in.h > 0 && in.w <= 65535 && in.h <= 65535, fn);
    VS_TRY(bgr_format_ok(format));
    VS_ARG_AS(ptrs && in.n >= 1 && in.stride >= in.w * 3 && (!out || out->stride >= out->w * out->channels), fn);
    return VS_OK;
}
// what an index-based wrapper asks on top of its pass's rule: the batch the indices point into, and the indices (behind_end: CandIndex::check)
int indexed_args_ok(const char* fn, const plan::Batch& in, const plan::CandIndex& idx, bool behind_end) {
    VS_ARG_AS(in.p && idx.cand_frame && in.n >= 1 && in.strides_ok(), fn);
    VS_ARG_AS(idx.check(in.n, behind_end), fn);
    return VS_OK;
}

int deblur_params_ok(const vs_deblur_params* params, vs_deblur_params* p) {
    if (params) *p = *params; else vs_deblur_params_default(p);
    VS_ARG(deblur_params_finite(p->sensitivity, p->max_ratio));      // (the box and max_ratio^2 / sensitivity <= 2^100: the fp32 sums stay finite)
    return VS_OK;
}
int denoise_params_ok(const vs_denoise_params* params, vs_denoise_params* p) {
    if (params) *p = *params; else vs_denoise_params_default(p);
    VS_ARG(denoise_params_valid(*p));
    return VS_OK;
}
int rolling_params_ok(const vs_rolling_params* params, vs_rolling_params* p) {
    if (params) *p = *params; else vs_rolling_params_default(p);
    VS_ARG(rolling_params_valid(*p));
    return VS_OK;
}
int deflicker_params_ok(const vs_deflicker_params* params, vs_deflicker_params* p) {
    if (params) *p = *params; else vs_deflicker_params_default(p);
    VS_ARG(deflicker_params_valid(*p));
    return VS_OK;
}

// the callbacks of cand_groups for a pass whose entry 0 is the frame itself, which has to be there, and whose other entries have no side word
struct FrameIsEntry0 {
    const void* const* cand_src;
    int n_cand;
    const char* fn;
    int operator()(vsk::FillCand& e, int o) const {
        VS_ARG_AS(cand_src[(size_t)o * n_cand], fn);
        e.src = cand_src[(size_t)o * n_cand];
        return VS_OK;
    }
};
bool no_side_word(vsk::FillCand&, size_t) { return true; }
// every target (entry 0) of the group's frames starts on a dword
bool targets_aligned(const void* const* cand_src, int f0, int nf, int n_cand) {
    for (int o = f0; o < f0 + nf; o++) if ((uintptr_t)cand_src[(size_t)o * n_cand] & 3) return false;
    return true;
}
int no_ring() { return set_error(VS_ERR_HIP, "no parameter ring for this device"); }
}  // namespace

// ---- deblur by transfer (vs_deblur.hip) ----
// The deblur pass on device-resident frames (vs_internal.hpp).  The list also ends at a frame without a sharpness pointer; entries and ratios
// together stay inside half the ring.
int vsi::bgr_deblur_ptrs(int n_out, int w, int h, int src_stride, int format, int n_cand, const void* const* cand_src, const uint64_t* const* cand_sharp,
                         const vs_transform* cand_t, const vs_deblur_params* params, void* dst, size_t dst_fs, int dst_stride, hipStream_t s) {
    const int bits = vs_format_bits(format);
    const plan::Batch out{dst, dst_fs, n_out, w, h, dst_stride, 3, bits};
    VS_TRY(pass_args_ok(__func__, nullptr, nullptr, w, h, format, n_cand, cand_src && cand_sharp && cand_t && dst, n_out, src_stride, &out));
    vs_deblur_params p;
    VS_TRY(deblur_params_ok(params, &p));
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const size_t esz = plan::elem_size(bits);
    const char* const fn = __func__;
    std::vector<vsk::DeblurCand> dc;
    return cand_groups(ring, 0, n_out, plan::frames_per_group_entries(n_cand, 5), n_cand, cand_src, cand_t, w, h, true, true, s, dc,
        [&](vsk::DeblurCand& e, int o) -> int {
            const size_t base = (size_t)o * n_cand;
            VS_ARG_AS(cand_src[base] && cand_sharp[base], fn);
            e.src = cand_src[base];
            e.sharp = (const unsigned long long*)cand_sharp[base];
            return VS_OK;
        },
        [&](vsk::DeblurCand& e, size_t k) { return (e.sharp = (const unsigned long long*)cand_sharp[k]) != nullptr; },
        [&](vsk::DeblurCand* cdev, float* rdev, int f0, int nf) -> int {
            VS_HIP(vsk::bgr_deblur(cdev, rdev, n_cand, w, h, src_stride, (int)esz * 8, bits - 8, vs_format_max_value(format), p.sensitivity, p.max_ratio,
                                   (char*)dst + (size_t)f0 * dst_fs * esz, dst_stride, nf, dst_fs, targets_aligned(cand_src, f0, nf, n_cand), s));
            return VS_OK;
        });
}

// ---- motion-compensated temporal denoise (vs_denoise.hip) ----
// The denoise pass on device-resident frames (vs_internal.hpp), in groups of (kSlots / 2 / 4) / n_cand output frames: a group stays inside half the ring.
int vsi::bgr_denoise_ptrs(int n_out, int w, int h, int src_stride, int format, int n_cand, const void* const* cand_src, const vs_transform* cand_t,
                          const vs_denoise_params* params, void* dst, size_t dst_fs, int dst_stride, hipStream_t s) {
    const int bits = vs_format_bits(format);
    const plan::Batch out{dst, dst_fs, n_out, w, h, dst_stride, 3, bits};
    VS_TRY(pass_args_ok(__func__, "denoise", kCvShort, w, h, format, n_cand, cand_src && cand_t && dst, n_out, src_stride, &out));
    vs_denoise_params p;
    VS_TRY(denoise_params_ok(params, &p));
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const size_t esz = plan::elem_size(bits);
    std::vector<vsk::FillCand> dc;
    return cand_groups(ring, 0, n_out, plan::frames_per_group_entries(n_cand, 4), n_cand, cand_src, cand_t, w, h, false, true, s, dc,
        FrameIsEntry0{cand_src, n_cand, __func__}, no_side_word,
        [&](vsk::FillCand* cdev, float*, int f0, int nf) -> int {
            VS_HIP(vsk::bgr_denoise(cdev, n_cand, w, h, src_stride, (int)esz * 8, bits - 8, vs_format_max_value(format), p.strength,
                                    (char*)dst + (size_t)f0 * dst_fs * esz, dst_stride, nf, dst_fs, targets_aligned(cand_src, f0, nf, n_cand), s));
            return VS_OK;
        });
}

// ---- rolling-shutter correction (vs_rolling.hip) ----
// The rolling-shutter pass on device-resident frames (vs_internal.hpp); two entries per frame, in the denoise's groups.  Entry 1's frame pointer
// only says whether a motion is known: the kernel never follows it.
int vsi::bgr_rolling_ptrs(int n_out, int w, int h, int src_stride, int format, const void* const* cand_src, const vs_transform* cand_t,
                          const vs_rolling_params* params, void* dst, size_t dst_fs, int dst_stride, hipStream_t s) {
    const int bits = vs_format_bits(format);
    const plan::Batch out{dst, dst_fs, n_out, w, h, dst_stride, 3, bits};
    VS_TRY(pass_args_ok(__func__, "rolling shutter", kCvShort, w, h, format, 2, cand_src && cand_t && dst, n_out, src_stride, &out));
    vs_rolling_params p;
    VS_TRY(rolling_params_ok(params, &p));
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const size_t esz = plan::elem_size(bits);
    std::vector<vsk::FillCand> rc;
    return cand_groups(ring, 0, n_out, plan::frames_per_group_entries(2, 4), 2, cand_src, cand_t, w, h, false, true, s, rc,
        FrameIsEntry0{cand_src, 2, __func__}, no_side_word,
        [&](vsk::FillCand* cdev, float*, int f0, int nf) -> int {
            VS_HIP(vsk::bgr_rolling(cdev, w, h, src_stride, (int)esz * 8, vs_format_max_value(format), p.readout, (char*)dst + (size_t)f0 * dst_fs * esz,
                                    dst_stride, nf, dst_fs, s));
            return VS_OK;
        });
}

// ---- deflicker (vs_deflicker.hip) ----
// The statistics pass on device-resident frames (vs_internal.hpp); the entries travel in the denoise's groups.
int vsi::exposure_stats_ptrs(int n_out, int w, int h, int src_stride, int format, int n_cand, const void* const* cand_src, const vs_transform* cand_t,
                             const vs_deflicker_params* params, uint64_t* stats, hipStream_t s) {
    const int bits = vs_format_bits(format);
    VS_TRY(pass_args_ok(__func__, "deflicker", kAsTheFill, w, h, format, n_cand, cand_src && cand_t && stats, n_out, src_stride, nullptr));
    vs_deflicker_params p;
    VS_TRY(deflicker_params_ok(params, &p));
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const size_t esz = plan::elem_size(bits);
    std::vector<vsk::FillCand> dc;
    return cand_groups(ring, 0, n_out, plan::frames_per_group_entries(n_cand, 4), n_cand, cand_src, cand_t, w, h, false, true, s, dc,
        FrameIsEntry0{cand_src, n_cand, __func__}, no_side_word,
        [&](vsk::FillCand* cdev, float*, int f0, int nf) -> int {
            VS_HIP(vsk::exposure_stats(cdev, n_cand, w, h, src_stride, (int)esz * 8, bits - 8, p.step, (unsigned long long*)stats + (size_t)f0 * n_cand * 8, nf, s));
            return VS_OK;
        });
}

// ---- scene-cut detection (vs_scene.hip) ----
namespace {
int scene_params_ok(const vs_scene_params* params, vs_scene_params* p) {
    if (params) *p = *params; else vs_scene_params_default(p);
    VS_ARG(scene_params_valid(*p));
    return VS_OK;
}
}  // namespace

// The statistics pass on device-resident frames (vs_internal.hpp); two entries per pair, in the denoise's groups.
int vsi::scene_stats_ptrs(int n_pairs, int w, int h, int src_stride, int format, const void* const* pair_src, const vs_transform* pair_t,
                          const vs_scene_params* params, uint64_t* stats, hipStream_t s) {
    const int bits = vs_format_bits(format);
    VS_TRY(pass_args_ok(__func__, "scene cut", kAsTheFill, w, h, format, 2, pair_src && pair_t && stats, n_pairs, src_stride, nullptr));
    vs_scene_params p;
    VS_TRY(scene_params_ok(params, &p));
    for (int i = 0; i < n_pairs; i++) VS_ARG(pair_src[2 * (size_t)i] && pair_src[2 * (size_t)i + 1]);
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const size_t esz = plan::elem_size(bits);
    std::vector<vs_transform> t2((size_t)n_pairs * 2, vs_transform{0, 0, 0, 0});      // (entry 0's transform is not read)
    for (int i = 0; i < n_pairs; i++) t2[2 * (size_t)i + 1] = pair_t[i];
    std::vector<vsk::FillCand> pc;
    return cand_groups(ring, 0, n_pairs, plan::frames_per_group_entries(2, 4), 2, pair_src, t2.data(), w, h, false, true, s, pc,
        FrameIsEntry0{pair_src, 2, __func__}, no_side_word,
        [&](vsk::FillCand* cdev, float*, int f0, int nf) -> int {
            VS_HIP(vsk::scene_stats(cdev, w, h, src_stride, (int)esz * 8, bits - 8, vs_format_max_value(format), p.step,
                                    (unsigned long long*)stats + (size_t)f0 * 2, nf, s));
            return VS_OK;
        });
}

// ---- inpaint of what the fill leaves open (vs_inpaint.hip) ----
namespace {
// the coverage index's argument rule, for the function on the device and its index-based wrapper alike
int coverage_args_ok(const char* fn, int w, int h, int n_cand, bool ptrs, int n_out, int roi_x, int roi_y, int roi_w, int roi_h, size_t cov_fs, int cov_stride) {
    VS_ARG_AS(w > 0 && h > 0 && n_cand >= 1 && n_cand <= 16, fn);
    VS_TRY(lookahead_args_ok("fill coverage", kAsTheFill, w, h, n_cand));
    VS_ARG_AS(ptrs && n_out >= 1, fn);
    VS_ARG_AS(plan::window_ok(roi_x, roi_y, roi_w, roi_h, w, h), fn);
    VS_ARG_AS((plan::Batch{nullptr, cov_fs, n_out, roi_w, roi_h, cov_stride, 1, 8}).strides_ok(), fn);
    return VS_OK;
}
}  // namespace

// The coverage index on the device (vs_internal.hpp); the entries travel in the denoise's groups.  Entry 0 carries the frame's own matrix.
int vsi::fill_coverage_ptrs(int n_out, int w, int h, int n_cand, const void* const* cand_src, const vs_transform* cand_t, int roi_x, int roi_y, int roi_w,
                            int roi_h, uint8_t* cov, size_t cov_fs, int cov_stride, uint32_t* open_count, hipStream_t s, const char* fn) {
    VS_TRY(coverage_args_ok(fn, w, h, n_cand, cand_src && cand_t && cov, n_out, roi_x, roi_y, roi_w, roi_h, cov_fs, cov_stride));
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const vsk::Roi roi{roi_x, roi_y, roi_w, roi_h};
    std::vector<vsk::FillCand> fc;
    return cand_groups(ring, 0, n_out, plan::frames_per_group_entries(n_cand, 4), n_cand, cand_src, cand_t, w, h, false, true, s, fc,
        [&](vsk::FillCand& e, int o) -> int {
            vs_cv_inverse_matrix(&cand_t[(size_t)o * n_cand], w, h, e.m);
            return VS_OK;
        },
        no_side_word,
        [&](vsk::FillCand* cdev, float*, int f0, int nf) -> int {
            VS_HIP(vsk::fill_coverage(cdev, n_cand, w, h, cov + (size_t)f0 * cov_fs, cov_stride, nf, cov_fs, roi, open_count ? open_count + f0 : nullptr, s));
            return VS_OK;
        });
}

// ---- phase-compensated sharpening (vs_sharpen.hip) ----
namespace {
int sharpen_params_ok(const vs_sharpen_params* params, vs_sharpen_params* p) {
    if (params) *p = *params; else vs_sharpen_params_default(p);
    VS_ARG(sharpen_params_valid(*p));
    return VS_OK;
}
// the sharpen's argument rule, for the function on the device and its staging wrapper alike; none of it needs a device
int sharpen_args_ok(const char* fn, const plan::Batch& in, const plan::Batch& out, int w, int h, int format, const vs_transform* t, int roi_x, int roi_y) {
    VS_ARG_AS(w > 0 && h > 0 && w <= 65535 && h <= 65535 && in.n >= 0, fn);
    VS_TRY(bgr_format_ok(format));
    VS_TRY(lookahead_args_ok("sharpen", kAsTheFill, w, h, 1));
    VS_ARG_AS(plan::window_ok(roi_x, roi_y, in.w, in.h, w, h), fn);
    if (in.n == 0) return VS_OK;
    VS_ARG_AS(in.p && out.p && t, fn);
    VS_ARG_AS(in.strides_ok() && out.strides_ok(), fn);
    // the stencil cannot run in place
    const char *a0 = (const char*)in.p, *a1 = a0 + in.bytes(), *b0 = (const char*)out.p, *b1 = b0 + out.bytes();
    VS_ARG_AS(a1 <= b0 || b1 <= a0, fn);
    return VS_OK;
}
}  // namespace

// The sharpen pass on device-resident windows (vs_internal.hpp).  The frames' matrices travel through the parameter ring, three slots a frame, in
// the plain warp's groups.
int vsi::bgr_sharpen_ptrs(const void* src, size_t src_fs, int n, int w, int h, int format, const vs_transform* t, const vs_sharpen_params* params, int roi_x,
                          int roi_y, int roi_w, int roi_h, int src_stride, void* dst, size_t dst_fs, int dst_stride, hipStream_t s) {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, roi_w, roi_h, src_stride, 3, bits}, out{dst, dst_fs, n, roi_w, roi_h, dst_stride, 3, bits};
    VS_TRY(sharpen_args_ok(__func__, in, out, w, h, format, t, roi_x, roi_y));
    vs_sharpen_params p;
    VS_TRY(sharpen_params_ok(params, &p));
    if (n == 0) return VS_OK;
    ParamRing* ring = param_ring();
    if (!ring) return no_ring();
    const size_t esz = in.esz();
    const int per_call = plan::frames_per_group_matrices();
    std::vector<double> Mv((size_t)std::min(n, per_call) * 6);
    for (int f0 = 0; f0 < n; f0 += per_call) {
        const int nf = std::min(per_call, n - f0);
        for (int i = 0; i < nf; i++) vs_cv_inverse_matrix(&t[f0 + i], w, h, &Mv[(size_t)i * 6]);
        float4* mdev = nullptr;
        VS_TRY(send_slots(ring, Mv.data(), (size_t)nf * 3, s, &mdev));             // (six doubles: three 16-byte slots)
        VS_HIP(vsk::bgr_sharpen((const char*)src + (size_t)f0 * src_fs * esz, src_fs, nf, w, h, src_stride, (int)esz * 8, vs_format_max_value(format),
                                (const double*)mdev, p.strength, vsk::Roi{roi_x, roi_y, roi_w, roi_h}, (char*)dst + (size_t)f0 * dst_fs * esz, dst_fs, dst_stride, s));
        VS_TRY(ring->fence(mdev, s));
    }
    return VS_OK;
}

extern "C" {

int vs_bgr_channel_sums_batch(const void* src, size_t src_fs, int n, int w, int h, int src_stride, int format, uint64_t* sums, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, w, h, src_stride, 3, bits};
    VS_TRY(batch_args_ok(__func__, format, src && sums, in, nullptr));
    if (w > 32767 || h > 32767) return set_error(VS_ERR_UNSUPPORTED, "channel sums: frames up to 32767 x 32767, as the border fill");
    VS_ARG(in.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(o.out(sums, (size_t)n * 3 * sizeof(uint64_t), mem));
    VS_HIP(vsk::bgr_channel_sums(a.dev, w, h, src_stride, (int)in.esz() * 8, o.as<unsigned long long>(), n, src_fs, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_sharpness_batch(const void* src, size_t src_fs, int n, int w, int h, int src_stride, int format, uint64_t* sharpness, int mem,
                           void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, w, h, src_stride, 3, bits};
    VS_TRY(batch_args_ok(__func__, format, src && sharpness, in, nullptr));
    VS_ARG(in.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(o.out(sharpness, (size_t)n * sizeof(uint64_t), mem));
    VS_HIP(vsk::bgr_sharpness(a.dev, w, h, src_stride, (int)in.esz() * 8, bits - 8, o.as<unsigned long long>(), n, src_fs, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_deblur_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int format, const uint64_t* sharpness, int n_out,
                        int n_cand, const int32_t* cand_frame, const vs_transform* cand_t, const vs_deblur_params* params, void* dst, size_t dst_fs,
                        int dst_stride, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n_src, w, h, src_stride, 3, bits}, out{dst, dst_fs, n_out, w, h, dst_stride, 3, bits};
    const plan::CandIndex idx{cand_frame, n_out, n_cand};
    VS_TRY(pass_args_ok(__func__, nullptr, nullptr, w, h, format, n_cand, sharpness && cand_frame && cand_t && dst, n_out, src_stride, &out));
    VS_TRY(indexed_args_ok(__func__, in, idx, true));
    vs_deblur_params p;
    VS_TRY(deblur_params_ok(params, &p));
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, sh, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(sh.in(sharpness, (size_t)n_src * sizeof(uint64_t), mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    const std::vector<const void*> ptrs = idx.pointers<void>(a.dev, src_fs * in.esz());
    const std::vector<const uint64_t*> sharp = idx.pointers<uint64_t>(sh.dev, sizeof(uint64_t));
    VS_TRY(bgr_deblur_ptrs(n_out, w, h, src_stride, format, n_cand, ptrs.data(), sharp.data(), cand_t, &p, o.dev, dst_fs, dst_stride, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_denoise_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int format, int n_out, int n_cand,
                         const int32_t* cand_frame, const vs_transform* cand_t, const vs_denoise_params* params, void* dst, size_t dst_fs, int dst_stride,
                         int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n_src, w, h, src_stride, 3, bits}, out{dst, dst_fs, n_out, w, h, dst_stride, 3, bits};
    const plan::CandIndex idx{cand_frame, n_out, n_cand};
    VS_TRY(pass_args_ok(__func__, "denoise", kCvShort, w, h, format, n_cand, cand_frame && cand_t && dst, n_out, src_stride, &out));
    VS_TRY(indexed_args_ok(__func__, in, idx, false));
    vs_denoise_params p;
    VS_TRY(denoise_params_ok(params, &p));
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    const std::vector<const void*> ptrs = idx.pointers<void>(a.dev, src_fs * in.esz());
    VS_TRY(bgr_denoise_ptrs(n_out, w, h, src_stride, format, n_cand, ptrs.data(), cand_t, &p, o.dev, dst_fs, dst_stride, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_rolling_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int format, int n_out, const int32_t* cand_frame,
                         const vs_transform* cand_t, const vs_rolling_params* params, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n_src, w, h, src_stride, 3, bits}, out{dst, dst_fs, n_out, w, h, dst_stride, 3, bits};
    VS_TRY(pass_args_ok(__func__, "rolling shutter", kCvShort, w, h, format, 2, cand_frame && cand_t && dst, n_out, src_stride, &out));
    // only the sign of entry 1's index is looked at: a live entry 1 stands for the frame itself, whose pointer is never followed
    std::vector<int32_t> live((size_t)n_out * 2);
    for (int o = 0; o < n_out; o++) {
        live[2 * (size_t)o] = cand_frame[2 * (size_t)o];
        live[2 * (size_t)o + 1] = cand_frame[2 * (size_t)o + 1] >= 0 ? cand_frame[2 * (size_t)o] : -1;
    }
    const plan::CandIndex idx{live.data(), n_out, 2};
    VS_TRY(indexed_args_ok(__func__, in, idx, false));
    vs_rolling_params p;
    VS_TRY(rolling_params_ok(params, &p));
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    const std::vector<const void*> ptrs = idx.pointers<void>(a.dev, src_fs * in.esz());
    VS_TRY(bgr_rolling_ptrs(n_out, w, h, src_stride, format, ptrs.data(), cand_t, &p, o.dev, dst_fs, dst_stride, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

// ---- remap and the radial lens map (vs_remap.hip) ----
int vs_lens_map(const vs_lens_params* p, int w, int h, int32_t* map, int map_stride, int mem, void* stream) try {
    if (mem == VS_MEM_HOST) return lens_map_host(p, w, h, map, map_stride);
    VS_ARG(mem == VS_MEM_DEVICE);
    VS_ARG(p && map && w >= 1 && h >= 1 && w <= 32767 && h <= 32767 && map_stride >= 2 * w && vsl::params_ok(*p));
    if (!device_ready()) return VS_ERR_HIP;
    VS_HIP(vsk::lens_map(*p, w, h, map, map_stride, (hipStream_t)stream));
    return VS_OK;
} VS_CATCH_ALL

int vs_bgr_remap_batch(const void* src, size_t src_fs, int n, int w, int h, int src_stride, int format, const int32_t* map, int map_stride, int ow, int oh,
                       int border, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, w, h, src_stride, 3, bits}, out{dst, dst_fs, n, ow, oh, dst_stride, 3, bits};
    VS_TRY(batch_args_ok(__func__, format, src && map && dst, in, &out));
    VS_ARG(ow > 0 && oh > 0 && ow <= 65535 && oh <= 65535 && map_stride >= 2 * ow && (border == VS_BORDER_CLAMP || border == VS_BORDER_CONSTANT));
    if (w > 32767 || h > 32767 || ow > 32767 || oh > 32767) return set_error(VS_ERR_UNSUPPORTED, "remap: frames and maps up to 32767 x 32767%s", kAsTheFill);
    VS_ARG(in.strides_ok() && out.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    // how many frames a workgroup takes a pixel through: tools/lens_bench.py times other lengths through the test hooks
    const char* const hook = test_env("VS_TEST_REMAP_SLICE");
    const int slice = hook && atoi(hook) >= 1 ? atoi(hook) : vsk::kRemapSlice;
    Staged a, m, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(m.in(map, ((size_t)(oh - 1) * (size_t)map_stride + 2 * (size_t)ow) * sizeof(int32_t), mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    VS_HIP(vsk::bgr_remap(a.dev, src_fs, n, w, h, src_stride, (int)in.esz() * 8, vs_format_max_value(format), m.as<int32_t>(), map_stride, ow, oh, border, o.dev,
                          dst_fs, dst_stride, slice, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_exposure_stats_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int format, int n_out, int n_cand,
                                const int32_t* cand_frame, const vs_transform* cand_t, const vs_deflicker_params* params, uint64_t* stats, int mem,
                                void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n_src, w, h, src_stride, 3, bits};
    const plan::CandIndex idx{cand_frame, n_out, n_cand};
    VS_TRY(pass_args_ok(__func__, "deflicker", kAsTheFill, w, h, format, n_cand, stats && cand_frame && cand_t, n_out, src_stride, nullptr));
    VS_TRY(indexed_args_ok(__func__, in, idx, false));
    vs_deflicker_params p;
    VS_TRY(deflicker_params_ok(params, &p));
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(o.out(stats, (size_t)n_out * n_cand * 8 * sizeof(uint64_t), mem));
    const std::vector<const void*> ptrs = idx.pointers<void>(a.dev, src_fs * in.esz());
    VS_TRY(exposure_stats_ptrs(n_out, w, h, src_stride, format, n_cand, ptrs.data(), cand_t, &p, o.as<uint64_t>(), s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_scene_stats_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int format, int n_pairs, const int32_t* pair_frames,
                             const vs_transform* pair_t, const vs_scene_params* params, uint64_t* stats, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n_src, w, h, src_stride, 3, bits};
    VS_ARG(n_pairs >= 0);
    VS_TRY(pass_args_ok(__func__, "scene cut", kAsTheFill, w, h, format, 2, src != nullptr, 1, src_stride, nullptr));
    VS_ARG(n_src >= 1 && in.strides_ok());
    vs_scene_params p;
    VS_TRY(scene_params_ok(params, &p));
    if (n_pairs == 0) return VS_OK;                                     // nothing to measure, nothing launched
    VS_ARG(pair_frames && pair_t && stats);
    for (size_t i = 0; i < 2 * (size_t)n_pairs; i++) VS_ARG(pair_frames[i] >= 0 && pair_frames[i] < n_src);
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(o.out(stats, (size_t)n_pairs * 2 * sizeof(uint64_t), mem));
    std::vector<const void*> ptrs(2 * (size_t)n_pairs);
    for (size_t i = 0; i < ptrs.size(); i++) ptrs[i] = (const char*)a.dev + (size_t)pair_frames[i] * src_fs * in.esz();
    VS_TRY(scene_stats_ptrs(n_pairs, w, h, src_stride, format, ptrs.data(), pair_t, &p, o.as<uint64_t>(), s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_exposure_gains_batch(const uint64_t* stats, int n_out, int n_cand, int w, int h, const vs_deflicker_params* params, uint32_t* gains, int mem,
                            void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(stats && gains && n_out >= 1 && n_cand >= 1 && n_cand <= 16);
    vs_deflicker_params p;
    VS_TRY(deflicker_params_ok(params, &p));
    if (mem == VS_MEM_HOST)                                             // the rule's bounds, where the host can see them
        for (size_t e = 0; e < (size_t)n_out * n_cand; e++) {
            VS_ARG(stats[e * 8] < (1ull << 30));
            for (int k = 1; k < 7; k++) VS_ARG(stats[e * 8 + k] < (1ull << 46));
        }
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(a.in(stats, (size_t)n_out * n_cand * 8 * sizeof(uint64_t), mem, s));
    VS_TRY(o.out(gains, (size_t)n_out * 4 * sizeof(uint32_t), mem));
    VS_HIP(vsk::exposure_gains(a.as<unsigned long long>(), n_out, n_cand, w, h, p.step, o.as<uint32_t>(), s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_gain_batch(const void* src, size_t src_fs, int n, int w, int h, int src_stride, int format, const uint32_t* gains, void* dst, size_t dst_fs,
                      int dst_stride, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, w, h, src_stride, 3, bits}, out{dst, dst_fs, n, w, h, dst_stride, 3, bits};
    VS_TRY(batch_args_ok(__func__, format, src && dst && gains, in, &out));
    VS_ARG(in.strides_ok() && out.strides_ok());
    if (mem == VS_MEM_HOST)
        for (size_t i = 0; i < (size_t)n; i++)
            for (int c = 0; c < 3; c++) VS_ARG(gains[4 * i + c] >= 16384u && gains[4 * i + c] <= 65536u);
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, g, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(g.in(gains, (size_t)n * 4 * sizeof(uint32_t), mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    VS_HIP(vsk::bgr_gain(a.dev, w, h, src_stride, (int)in.esz() * 8, vs_format_max_value(format), g.as<uint32_t>(), o.dev, dst_stride, n, src_fs, dst_fs, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_fill_coverage_batch(int w, int h, int n_out, int n_cand, const int32_t* cand_frame, const vs_transform* cand_t, int roi_x, int roi_y, int roi_w,
                               int roi_h, uint8_t* cov, size_t cov_frame_stride, int cov_stride, int mem, void* stream) try {
    VS_DIMS(w, h);
    VS_TRY(coverage_args_ok(__func__, w, h, n_cand, cand_frame && cand_t && cov, n_out, roi_x, roi_y, roi_w, roi_h, cov_frame_stride, cov_stride));
    for (int o = 0; o < n_out; o++) VS_ARG(cand_frame[(size_t)o * n_cand] >= 0);       // candidate 0 is the frame itself
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged o;
    VS_TRY(stage_out(o, plan::Batch{cov, cov_frame_stride, n_out, roi_w, roi_h, cov_stride, 1, 8}, mem, 1));
    // only the sign of an index is looked at: a live entry gets a frame pointer that is never followed
    static const char live = 0;
    std::vector<const void*> ptrs((size_t)n_out * n_cand, nullptr);
    for (int i = 0; i < n_out; i++)
        for (int c = 0; c < n_cand && cand_frame[(size_t)i * n_cand + c] >= 0; c++) ptrs[(size_t)i * n_cand + c] = &live;
    VS_TRY(fill_coverage_ptrs(n_out, w, h, n_cand, ptrs.data(), cand_t, roi_x, roi_y, roi_w, roi_h, o.as<uint8_t>(), cov_frame_stride, cov_stride, nullptr, s,
                              __func__));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_inpaint_batch(void* img, size_t frame_stride, int n, int w, int h, int stride, int format, const uint8_t* mask, size_t mask_frame_stride,
                         int mask_stride, int mem, void* stream) try {
    VS_DIMS(w, h);
    const int bits = vs_format_bits(format);
    VS_TRY(bgr_format_ok(format));
    if (w > 32767 || h > 32767) return set_error(VS_ERR_UNSUPPORTED, "inpaint: windows up to 32767 x 32767%s", kAsTheFill);
    const plan::Batch frames{img, frame_stride, n, w, h, stride, 3, bits}, masks{mask, mask_frame_stride, n, w, h, mask_stride, 1, 8};
    VS_ARG(img && mask && n >= 1 && stride >= w * 3 && mask_stride >= w);
    VS_ARG(frames.strides_ok() && masks.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = frames.esz();
    Staged a, m, o;
    VS_TRY(stage_in(a, frames, mem, s));
    VS_TRY(stage_in(m, masks, mem, s));
    VS_TRY(stage_out(o, frames, mem, esz));
    if (o.dev != a.dev) VS_HIP(hipMemcpyAsync(o.dev, a.dev, frames.bytes(), hipMemcpyDeviceToDevice, s));      // host memory: the windows are worked on in the output's block
    // the open counts, then the pyramid (8-byte aligned behind them), in one block that lives until the work on `s` is done
    const size_t cbytes = ((size_t)n * sizeof(unsigned int) + 255) & ~(size_t)255;
    DevBuf scratch;
    VS_HIP(scratch.alloc(cbytes + (size_t)n * vsk::inpaint_pyramid_bytes(w, h, (int)esz * 8)));
    VS_HIP(vsk::mask_open_count(m.as<uint8_t>(), w, h, mask_stride, mask_frame_stride, n, scratch.as<unsigned int>(), s));
    VS_HIP(vsk::bgr_inpaint(o.dev, frame_stride, n, w, h, stride, (int)esz * 8, m.as<uint8_t>(), mask_frame_stride, mask_stride, scratch.as<unsigned int>(),
                            scratch.as<char>() + cbytes, s));
    const int r = finish_outputs(mem, s, {&o});
    if (mem != VS_MEM_HOST) VS_HIP(hipStreamSynchronize(s));             // (the scratch is released on return)
    return r;
} VS_CATCH_ALL

int vs_bgr_sharpen_batch(const void* src, size_t src_fs, int n, int w, int h, int format, const vs_transform* t, const vs_sharpen_params* params, int roi_x,
                         int roi_y, int roi_w, int roi_h, int src_stride, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream) try {
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, roi_w, roi_h, src_stride, 3, bits}, out{dst, dst_fs, n, roi_w, roi_h, dst_stride, 3, bits};
    VS_ARG(mem == VS_MEM_HOST || mem == VS_MEM_DEVICE);
    VS_TRY(sharpen_args_ok(__func__, in, out, w, h, format, t, roi_x, roi_y));
    vs_sharpen_params p;
    VS_TRY(sharpen_params_ok(params, &p));
    if (n == 0) return VS_OK;                                           // nothing to sharpen, nothing launched
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    VS_TRY(bgr_sharpen_ptrs(a.dev, src_fs, n, w, h, format, t, &p, roi_x, roi_y, roi_w, roi_h, src_stride, o.dev, dst_fs, dst_stride, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

}  // extern "C"
