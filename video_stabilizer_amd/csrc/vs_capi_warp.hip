// vs_capi_warp.hip -- the frame warp of the C ABI (include/vs_amd.h): vs_bgr_image_warp and its batch / window / float forms, and the border
// fill behind the VS_WARP_BILINEAR_CV warp.  One checked call (WarpCall), two routes: the fixed-point route (cv::warpAffine's arithmetic, in
// launch groups, with the fill's pass 2 per group) and the tiled Lanczos2 / bilinear route (one launch).
#include "vs_capi.hpp"

using namespace vsi;

namespace {
// Border fill behind the VS_WARP_BILINEAR_CV warp (vs_fill.hip): per output frame n_cand candidates, host arrays of n_frames * n_cand entries.
// src[o * n_cand + c], c >= 1: the candidate's frame in device memory (w x h, rows of src_stride elements; null ends the list); entry c == 0 is
// the frame itself and is not read.  t[o * n_cand + c]: its forward transform (entry 0 is what the frame is warped with).
// The blend (vs_fill.hip, THE BLEND RULE): feather / match as in vs_fill_blend_params; sums[o * n_cand + c] (match only): where the three channel
// sums of that candidate's ORIGINAL frame lie in device memory (entry 0: the output frame's).  Both switches off: the fill as it always was.
struct FillSpec { int n_cand; const void* const* src; const vs_transform* t; const uint64_t* const* sums = nullptr; int feather = 0, match = 0; };

// a warp call whose arguments have been checked: src.n frames at src, each warped by its t[i] into the window roi, which is all that dst holds
struct WarpCall {
    plan::Batch src;
    const vs_transform* t;
    int mode, border, max_value;
    plan::Batch dst;                             // (the window's extent; elements of osz() bytes)
    bool f32out;
    int mem;
    hipStream_t s;
    vsk::Roi roi;
    const FillSpec* fill;
    size_t esz() const { return src.esz(); }
    size_t osz() const { return f32out ? 4 : esz(); }
    int stage(Staged& a, Staged& o) const {
        VS_TRY(stage_in(a, src, mem, s));
        return stage_out(o, dst, mem, osz());
    }
};

// Pass 2 of the fill for one launch group of the fixed-point route, on the same stream: entry 0 carries the matrix pass 1 warped the frame with
// (M: the group's, six doubles a frame) and, with match, its sums; a group without a single candidate launches nothing.  dp: the group's output.
int fill_pass2(const WarpCall& c, ParamRing* ring, int f0, int nf, const double* M, char* dp, std::vector<vsk::FillCand>& fc) {
    const FillSpec& fill = *c.fill;
    const int nc = fill.n_cand, w = c.src.w, h = c.src.h;
    const bool blend = fill.feather > 0 || fill.match != 0;
    return cand_groups(ring, f0, nf, nf, nc, fill.src, fill.t, w, h, false, false, c.s, fc,
        [&](vsk::FillCand& e, int o) {
            memcpy(e.m, &M[(size_t)(o - f0) * 6], 6 * sizeof(double));
            if (fill.match) e.reserved = (unsigned long long)(uintptr_t)fill.sums[(size_t)o * nc];
            return VS_OK;
        },
        [&](vsk::FillCand& e, size_t k) {
            if (fill.match) e.reserved = (unsigned long long)(uintptr_t)fill.sums[k];
            else if (blend) e.reserved = vsk::fill_unit_gains();
            return true;
        },
        [&](vsk::FillCand* fdev, float*, int, int) -> int {
            if (blend)
                VS_HIP(vsk::bgr_warp_cv_fill_blend_c3(fdev, nc, w, h, c.src.stride, c.src.bits, c.max_value, fill.feather, fill.match != 0, dp, c.dst.stride, nf,
                                                      c.dst.fs, c.roi, c.s));
            else
                VS_HIP(vsk::bgr_warp_cv_fill_c3(fdev, nc, w, h, c.src.stride, c.src.bits, c.max_value, dp, c.dst.stride, nf, c.dst.fs, c.roi, c.s));
            return VS_OK;
        });
}

// One launch group of the fixed-point route: nf frames from sp into dp, their inverted matrices at M.  On the stream: the matrices' upload (none
// for a small call), the tables' take, table kernel and warp, the fences.
int warp_cv_group(const WarpCall& c, ParamRing* ring, TableRing* tring, size_t tab_per, int nf, const double* M, const char* sp, char* dp) {
    const plan::Batch& in = c.src;
    hipError_t e = hipErrorNotSupported;
    int* tdev = nullptr;
    float4* mdev = nullptr;
    const auto upload_matrices = [&]() { return ring->upload((const float4*)M, plan::matrix_slots((size_t)nf), c.s, &mdev); };
    // small calls (one frame of the drop-in pattern, the parity tests' batches): the matrices go to the table kernel as kernel arguments, no upload
    const bool by_value = in.n <= vsk::kCvInlineFrames;
    if (in.channels == 3 && tring && tab_per * (size_t)nf <= TableRing::kInts / 2) {
        if (!by_value) VS_TRY(upload_matrices());
        VS_TRY(tring->take(tab_per * (size_t)nf, c.s, &tdev));
        e = vsk::bgr_warp_cv_c3(sp, in.w, in.h, in.stride, in.bits, (const double*)mdev, by_value ? M : nullptr, tdev, c.border, c.max_value, dp, c.dst.stride, nf,
                                in.fs, c.dst.fs, c.roi, c.s);
    }
    if (e == hipErrorNotSupported) {
        if (!mdev) VS_TRY(upload_matrices());
        e = vsk::bgr_warp_cv_generic(sp, in.w, in.h, in.stride, in.channels, in.bits, (const double*)mdev, c.border, c.max_value, dp, c.dst.stride, nf, in.fs,
                                     c.dst.fs, c.roi, c.s);
    }
    VS_HIP(e);
    if (mdev) VS_TRY(ring->fence(mdev, c.s));
    if (tdev) VS_TRY(tring->fence(tdev, c.s));
    return VS_OK;
}

// VS_WARP_BILINEAR_CV, cv::warpAffine's own arithmetic: t[i] is the FORWARD transform; its inverted matrix (six doubles = three ring slots per
// frame) is what the kernels take.  Frames go in launch groups (plan::frames_per_group_cv): their matrices fit one upload of the parameter ring,
// with a fill their candidate entries too, and -- tuned kernel -- their coordinate tables half of the table ring.
int warp_cv_route(const WarpCall& c) {
    const plan::Batch& in = c.src;
    ParamRing* ring = param_ring();
    if (!ring) return set_error(VS_ERR_UNSUPPORTED, "no current HIP device with index < 16");
    Staged a, o;
    VS_TRY(c.stage(a, o));
    TableRing* tring = in.channels == 3 ? table_ring() : nullptr;
    const size_t tab_per = in.channels == 3 ? vsk::bgr_warp_cv_table_ints(in.bits, c.roi) : 0;
    const int per_call = plan::frames_per_group_cv(c.fill ? c.fill->n_cand : 0, tab_per);
    std::vector<vsk::FillCand> fc;
    std::vector<double> Mv((size_t)std::min(in.n, per_call) * 6 + 2);   // (+2: an upload is counted in 16-byte slots)
    for (int f0 = 0; f0 < in.n; f0 += per_call) {
        const int nf = std::min(per_call, in.n - f0);
        for (int i = 0; i < nf; i++) vs_cv_inverse_matrix(&c.t[f0 + i], in.w, in.h, &Mv[(size_t)i * 6]);
        char* dp = (char*)o.dev + (size_t)f0 * c.dst.fs * c.esz();
        VS_TRY(warp_cv_group(c, ring, tring, tab_per, nf, Mv.data(), (const char*)a.dev + (size_t)f0 * in.fs * c.esz(), dp));
        if (c.fill && c.fill->n_cand > 1) VS_TRY(fill_pass2(c, ring, f0, nf, Mv.data(), dp, fc));
    }
    return finish_outputs(c.mem, c.s, {&o});
}

// The tiled Lanczos2 / bilinear route: one launch over all frames.  On the stream: the kernel parameters (send_slots), the staged input, the
// tables' take, the warp, the fences.
int warp_tiled_route(const WarpCall& c) {
    const plan::Batch& in = c.src;
    const int n = in.n;
    // kernel parameters of every frame, then (tuned 3-channel kernel) the extents its tile prologue uses: one block of 2n float4
    const bool tuned = in.channels == 3 && !c.f32out && c.max_value >= 0 && c.max_value <= (in.bits == 8 ? 255 : 65535);
    const bool with_extents = tuned && (size_t)n * 2 <= ParamRing::kSlots / 2;   // (the ring takes half its slots per call)
    std::vector<float> P((size_t)n * (with_extents ? 8 : 4));
    float* const extents = P.data() + (size_t)n * 4;
    for (int i = 0; i < n; i++) vs_ul_params_warp(&c.t[i], in.w, in.h, &P[(size_t)i * 4]);
    if (with_extents) vsk::bgr_warp_c3_extents(P.data(), n, c.roi, in.bits, c.mode, extents);
    const int compact = with_extents && !warp_keeps_solver_slot() ? vsk::bgr_warp_c3_compact_shape(extents, n) : 0;
    // the parameters travel through the ring's device half, so a VS_MEM_DEVICE call stays asynchronous and never reads a host buffer that has
    // gone out of scope
    float4* pdev = nullptr;
    ParamRing* ring = param_ring();
    if (!ring) return set_error(VS_ERR_UNSUPPORTED, "no current HIP device with index < 16");
    VS_TRY(send_slots(ring, P.data(), P.size() / 4, c.s, &pdev));
    Staged a, o;
    VS_TRY(c.stage(a, o));
    // the float-tile Lanczos2 forms' per-launch tables (tile windows, row terms: vsk::bgr_warp_c3) from the table ring, 16-byte aligned; a call whose
    // tables do not fit half the ring goes without them (the kernel then works the same numbers out itself)
    int* tdev = nullptr;
    TableRing* tring = nullptr;
    const size_t tab_ints = with_extents ? vsk::bgr_warp_c3_table_bytes(in.bits, c.mode, c.roi) / 4 * (size_t)n : 0;
    if (plan::aligned_tables_fit(tab_ints) && (tring = table_ring())) VS_TRY(tring->take(plan::aligned_table_take(tab_ints), c.s, &tdev));
    void* const tab = tdev ? (void*)plan::align16((uintptr_t)tdev) : nullptr;
    hipError_t e = hipErrorNotSupported;
    if (tuned)
        e = vsk::bgr_warp_c3(a.dev, in.w, in.h, in.stride, in.bits, pdev, with_extents ? pdev + n : nullptr, tab, c.mode, c.border, c.max_value, o.dev,
                             c.dst.stride, n, in.fs, c.dst.fs, c.roi, compact, c.s);
    if (e == hipErrorNotSupported)   // layouts without a tuned kernel (other channel counts, float output): one thread per pixel, same arithmetic
        e = vsk::bgr_warp_generic(a.dev, in.w, in.h, in.stride, in.channels, in.bits, pdev, c.mode, c.border, c.max_value,
                                  o.dev, c.dst.stride, c.f32out, n, in.fs, c.dst.fs, c.roi, c.s);
    VS_HIP(e);
    VS_TRY(ring->fence(pdev, c.s));
    if (tdev) VS_TRY(tring->fence(tdev, c.s));
    return finish_outputs(c.mem, c.s, {&o});
}

// The checks of every warp call, then its route.  roi = NULL: the whole w x h output.  Otherwise dst holds only the window (roi->w x roi->h
// pixels per frame).
int bgr_warp_common(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int channels,
                    int bits, const vs_transform* t, int mode, int border, int max_value, void* dst,
                    size_t dst_fs, int dst_stride, bool f32out, int mem, hipStream_t s, const vsk::Roi* roi_in = nullptr,
                    const FillSpec* fill = nullptr) {
    VS_DIMS(w, h);
    VS_ARG(src && dst && t && n_frames >= 1 && w > 0 && h > 0 && channels >= 1 && channels <= 4);
    VS_ARG(bits == 8 || bits == 16);
    const vsk::Roi roi = roi_in ? *roi_in : vsk::Roi{0, 0, w, h};
    VS_ARG(plan::window_ok(roi.x, roi.y, roi.w, roi.h, w, h));
    const WarpCall c{{src, src_fs, n_frames, w, h, src_stride, channels, bits}, t, mode, border, max_value,
                     {dst, dst_fs, n_frames, roi.w, roi.h, dst_stride, channels, bits}, f32out, mem, s, roi, fill};
    VS_ARG(src_stride >= w * channels && dst_stride >= roi.w * channels);
    VS_ARG(mode == VS_WARP_LANCZOS2 || mode == VS_WARP_BILINEAR || mode == VS_WARP_LANCZOS2_FAST || mode == VS_WARP_LANCZOS2_SEP || mode == VS_WARP_BILINEAR_CV);
    VS_ARG(border == VS_BORDER_CLAMP || border == VS_BORDER_CONSTANT);
    if (mode == VS_WARP_BILINEAR_CV && f32out) return set_error(VS_ERR_UNSUPPORTED, "VS_WARP_BILINEAR_CV has integer outputs only (cv::warpAffine on 8- / 16-bit frames)");
    VS_ARG(c.src.strides_ok() && c.dst.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    if (mode != VS_WARP_BILINEAR_CV) return warp_tiled_route(c);
    VS_ARG(max_value >= 0 && max_value <= (bits == 8 ? 255 : 65535));
    return warp_cv_route(c);
}

int fill_blend_params_ok(const vs_fill_blend_params* params, vs_fill_blend_params* p) {
    *p = params ? *params : vs_fill_blend_params{0, 0};
    VS_ARG(fill_blend_params_valid(*p));
    return VS_OK;
}
}  // namespace

// cand_sums / blend: see FillSpec; blend == NULL or {0, 0}: the plain fill, launch for launch
int vsi::bgr_warp_fill_ptrs(const void* src, size_t src_fs, int n_out, int w, int h, int src_stride, int bits, int n_cand, const void* const* cand_src,
                            const vs_transform* cand_t, int border, int max_value, int roi_x, int roi_y, int roi_w, int roi_h, void* dst, size_t dst_fs,
                            int dst_stride, hipStream_t s, const uint64_t* const* cand_sums, const vs_fill_blend_params* blend) {
    VS_ARG(cand_src && cand_t && n_out >= 1);
    VS_TRY(lookahead_args_ok("border fill", kCvShort, w, h, n_cand));
    vs_fill_blend_params bp;
    VS_TRY(fill_blend_params_ok(blend, &bp));
    if (bp.match) {                                      // every candidate that has a frame has its sums
        VS_ARG(cand_sums);
        for (int o = 0; o < n_out; o++) {
            VS_ARG(cand_sums[(size_t)o * n_cand]);
            for (int c = 1; c < n_cand && cand_src[(size_t)o * n_cand + c]; c++) VS_ARG(cand_sums[(size_t)o * n_cand + c]);
        }
    }
    std::vector<vs_transform> t0((size_t)n_out);
    for (int o = 0; o < n_out; o++) t0[o] = cand_t[(size_t)o * n_cand];
    const vsk::Roi roi{roi_x, roi_y, roi_w, roi_h};
    const FillSpec fill{n_cand, cand_src, cand_t, cand_sums, bp.feather, bp.match};
    return bgr_warp_common(src, src_fs, n_out, w, h, src_stride, 3, bits, t0.data(), VS_WARP_BILINEAR_CV, border, max_value, dst, dst_fs, dst_stride, false,
                           VS_MEM_DEVICE, s, &roi, &fill);
}

// The index-based fill: the checks a host-memory call needs before anything is staged, then pass 1 and 2 for runs of outputs whose own frames
// are consecutive in the batch, one warp launch each (n_cand == 1 with frames 0 .. n-1 is vs_bgr_image_warp_roi_batch, launch for launch)
static int fill_batch_impl(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int channels, int bits, int n_out, int n_cand,
                           const int32_t* cand_frame, const vs_transform* cand_t, int border, int max_value, int roi_x, int roi_y, int roi_w,
                           int roi_h, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream, const uint64_t* sums, const vs_fill_blend_params* blend) {
    VS_DIMS(w, h);
    VS_ARG(src && dst && cand_frame && cand_t && n_src >= 1 && n_out >= 1 && (bits == 8 || bits == 16));
    VS_ARG(channels == 3);
    VS_TRY(lookahead_args_ok("border fill", kCvShort, w, h, n_cand));
    vs_fill_blend_params bp;
    VS_TRY(fill_blend_params_ok(blend, &bp));
    VS_ARG(sums || !bp.match);
    VS_ARG(plan::window_ok(roi_x, roi_y, roi_w, roi_h, w, h));
    const plan::Batch in{src, src_fs, n_src, w, h, src_stride, 3, bits}, out{dst, dst_fs, n_out, roi_w, roi_h, dst_stride, 3, bits};
    VS_ARG(in.strides_ok() && out.strides_ok());
    const plan::CandIndex idx{cand_frame, n_out, n_cand};
    VS_ARG(idx.check(n_src, true));
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t esz = in.esz();
    Staged a, sm, o;
    VS_TRY(stage_in(a, in, mem, s));
    if (bp.match) VS_TRY(sm.in(sums, (size_t)n_src * 3 * sizeof(uint64_t), mem, s));
    VS_TRY(stage_out(o, out, mem, esz));
    const std::vector<const void*> ptrs = idx.pointers<void>(a.dev, src_fs * esz);
    const std::vector<const uint64_t*> sptrs = bp.match ? idx.pointers<uint64_t>(sm.dev, 3 * sizeof(uint64_t)) : std::vector<const uint64_t*>();
    for (int j = 0, e; j < n_out; j = e) {
        e = idx.run_end(j);
        VS_TRY(bgr_warp_fill_ptrs(ptrs[(size_t)j * n_cand], src_fs, e - j, w, h, src_stride, bits, n_cand, &ptrs[(size_t)j * n_cand],
                                  &cand_t[(size_t)j * n_cand], border, max_value, roi_x, roi_y, roi_w, roi_h, (char*)o.dev + (size_t)j * dst_fs * esz,
                                  dst_fs, dst_stride, s, bp.match ? &sptrs[(size_t)j * n_cand] : nullptr, &bp));
    }
    return finish_outputs(mem, s, {&o});
}

extern "C" {

int vs_bgr_image_warp(const void* src, int w, int h, int src_stride, int channels, int bits, const vs_transform* t,
                      int mode, int border, int max_value, void* dst, int dst_stride, int mem, void* stream) try {
    return bgr_warp_common(src, 0, 1, w, h, src_stride, channels, bits, t, mode, border, max_value, dst, 0, dst_stride,
                           false, mem, (hipStream_t)stream);
} VS_CATCH_ALL

int vs_bgr_image_warp_batch(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int channels,
                            int bits, const vs_transform* t, int mode, int border, int max_value, void* dst,
                            size_t dst_fs, int dst_stride, int mem, void* stream) try {
    return bgr_warp_common(src, src_fs, n_frames, w, h, src_stride, channels, bits, t, mode, border, max_value, dst,
                           dst_fs, dst_stride, false, mem, (hipStream_t)stream);
} VS_CATCH_ALL

int vs_bgr_image_warp_roi_batch(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int channels,
                                int bits, const vs_transform* t, int mode, int border, int max_value, int roi_x, int roi_y,
                                int roi_w, int roi_h, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream) try {
    const vsk::Roi roi{roi_x, roi_y, roi_w, roi_h};
    return bgr_warp_common(src, src_fs, n_frames, w, h, src_stride, channels, bits, t, mode, border, max_value, dst,
                           dst_fs, dst_stride, false, mem, (hipStream_t)stream, &roi);
} VS_CATCH_ALL

int vs_bgr_image_warp_f32(const void* src, int w, int h, int src_stride, int channels, int bits, const vs_transform* t,
                          int mode, int border, float* dst, int dst_stride, int mem, void* stream) try {
    return bgr_warp_common(src, 0, 1, w, h, src_stride, channels, bits, t, mode, border, 0, dst, 0, dst_stride, true, mem,
                           (hipStream_t)stream);
} VS_CATCH_ALL

int vs_bgr_image_warp_fill_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int channels, int bits, int n_out, int n_cand,
                                 const int32_t* cand_frame, const vs_transform* cand_t, int border, int max_value, int roi_x, int roi_y, int roi_w,
                                 int roi_h, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream) try {
    return fill_batch_impl(src, src_fs, n_src, w, h, src_stride, channels, bits, n_out, n_cand, cand_frame, cand_t, border, max_value, roi_x, roi_y, roi_w, roi_h,
                           dst, dst_fs, dst_stride, mem, stream, nullptr, nullptr);
} VS_CATCH_ALL

int vs_bgr_image_warp_fill_blend_batch(const void* src, size_t src_fs, int n_src, int w, int h, int src_stride, int channels, int bits, int n_out, int n_cand,
                                       const int32_t* cand_frame, const vs_transform* cand_t, const uint64_t* sums, const vs_fill_blend_params* params,
                                       int border, int max_value, int roi_x, int roi_y, int roi_w, int roi_h, void* dst, size_t dst_fs, int dst_stride,
                                       int mem, void* stream) try {
    VS_ARG(params);
    return fill_batch_impl(src, src_fs, n_src, w, h, src_stride, channels, bits, n_out, n_cand, cand_frame, cand_t, border, max_value, roi_x, roi_y, roi_w, roi_h,
                           dst, dst_fs, dst_stride, mem, stream, sums, params);
} VS_CATCH_ALL

}  // extern "C"
