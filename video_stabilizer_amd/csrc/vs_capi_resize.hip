// vs_capi_resize.hip -- the resize pass at the C ABI (include/vs_amd.h): vs_resize_taps and vs_bgr_resize_batch.  The rule's tables:
// vs_resize.hpp; the kernels: vs_resize.hip.
#include "vs_capi.hpp"
#include "vs_resize.hpp"

using namespace vsi;

namespace {

// AREA outside its range, per axis, with the axis named
int area_range_ok(const char* fn, int filter, int sw, int sh, int dw, int dh) {
    if (filter != VS_RESIZE_AREA) return VS_OK;
    if (!vsr::resize_axis_valid(sw, dw, filter))
        return set_error(VS_ERR_UNSUPPORTED, "%s: VS_RESIZE_AREA needs dw <= sw <= 8 dw on the x axis (%d -> %d)", fn, sw, dw);
    if (!vsr::resize_axis_valid(sh, dh, filter))
        return set_error(VS_ERR_UNSUPPORTED, "%s: VS_RESIZE_AREA needs dh <= sh <= 8 dh on the y axis (%d -> %d)", fn, sh, dh);
    return VS_OK;
}

}  // namespace

extern "C" {

int vs_resize_taps(int s, int d, int filter, int32_t* i0, int32_t* n, uint16_t* wt) try {
    VS_ARG(i0 && n && wt && s >= 1 && d >= 1 && s <= vsr::kMaxExtent && d <= vsr::kMaxExtent);
    VS_ARG(filter == VS_RESIZE_LINEAR || filter == VS_RESIZE_AREA);
    if (!vsr::resize_axis_valid(s, d, filter)) return set_error(VS_ERR_UNSUPPORTED, "vs_resize_taps: VS_RESIZE_AREA needs d <= s <= 8 d (%d -> %d)", s, d);
    for (int k = 0; k < d; k++) {
        uint16_t* const w = wt + (size_t)k * vsr::kMaxTaps;
        std::fill(w, w + vsr::kMaxTaps, (uint16_t)0);
        int first = 0;
        n[k] = vsr::resize_taps(s, d, filter, k, &first, w);
        i0[k] = first;
    }
    return VS_OK;
} VS_CATCH_ALL

int vs_bgr_resize_batch(const void* src, size_t src_fs, int n, int sw, int sh, int src_stride, int format, int filter, void* dst, size_t dst_fs, int dw,
                        int dh, int dst_stride, int mem, void* stream) try {
    VS_DIMS(sw, sh);
    VS_DIMS(dw, dh);
    VS_TRY(bgr_format_ok(format));
    VS_ARG(n >= 0 && (filter == VS_RESIZE_LINEAR || filter == VS_RESIZE_AREA) && (mem == VS_MEM_HOST || mem == VS_MEM_DEVICE));
    if (sw > vsr::kMaxExtent || sh > vsr::kMaxExtent || dw > vsr::kMaxExtent || dh > vsr::kMaxExtent)
        return set_error(VS_ERR_UNSUPPORTED, "resize: frames up to 32767 x 32767 on both sides%s", kAsTheFill);
    VS_TRY(area_range_ok(__func__, filter, sw, sh, dw, dh));
    if (n == 0) return VS_OK;                                           // nothing to resize, nothing launched
    const int bits = vs_format_bits(format);
    const plan::Batch in{src, src_fs, n, sw, sh, src_stride, 3, bits}, out{dst, dst_fs, n, dw, dh, dst_stride, 3, bits};
    VS_ARG(src && dst && src != dst && in.strides_ok() && out.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    // which kernel form runs: tools/resize_bench.py and the bounds build's tests name one through the test hooks
    const char* const hook = test_env("VS_TEST_RESIZE_FORM");
    const int form = hook ? (atoi(hook) == vsk::kResizeDirect ? vsk::kResizeDirect : vsk::kResizeTiled) : vsk::kResizeAuto;
    TableRing* const tring = table_ring();
    if (!tring) return set_error(VS_ERR_UNSUPPORTED, "no current HIP device with index < 16");
    int* tdev = nullptr;
    Staged a, o;
    VS_TRY(stage_in(a, in, mem, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    VS_TRY(tring->take(vsk::resize_table_ints(dw, dh), s, &tdev));
    VS_HIP(vsk::bgr_resize(a.dev, src_fs, n, sw, sh, src_stride, (int)in.esz() * 8, vs_format_max_value(format), filter, tdev, o.dev, dst_fs, dw, dh, dst_stride,
                           form, s));
    VS_TRY(tring->fence(tdev, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

}  // extern "C"
