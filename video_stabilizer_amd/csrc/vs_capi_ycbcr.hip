// vs_capi_ycbcr.hip -- YCbCr frames at the C ABI (include/vs_amd.h): vs_ycbcr_to_bgr_batch, vs_bgr_to_ycbcr_batch and
// vs_stabilizer_process_batch_ycbcr.  The conversion is a pass of its own in front of and behind everything (vs_ycbcr.hip; the rule:
// vs_ycbcr.hpp): the stabilizer's entry point is a wrapper around vs_stabilizer_process_batch, not an engine change.
#include "vs_capi.hpp"
#include "vs_ycbcr.hpp"

#include <string>

using namespace vsi;

namespace {

// a descriptor's planes wherever the caller said: device memory as it is; host memory as staged spans, every plane one dense copy (an
// interleaved pair is one span).  dev: the descriptor the kernels take.
struct PlaneSet {
    Staged y, c, c2;
    vs_ycbcr_planes dev;
};
struct Span { void* p; size_t row_elems, rows, stride, fs; };
size_t span_bytes(const Span& sp, int n, size_t esz) { return ((size_t)(n - 1) * sp.fs + (sp.rows - 1) * sp.stride + sp.row_elems) * esz; }
// the spans of a descriptor's planes: Y, then the chroma run (planar: Cb, then Cr); returns how many
int spans_of(const vs_ycbcr_planes& pl, int w, int h, Span sp[3]) {
    sp[0] = Span{pl.y, (size_t)w, (size_t)h, (size_t)pl.y_stride, pl.y_frame_stride};
    if (!pl.cb) return 1;
    const size_t cw = (size_t)vsy::chroma_extent(w, pl.sub_x), ch = (size_t)vsy::chroma_extent(h, pl.sub_y);
    if (pl.c_step == 2) {
        sp[1] = Span{(uintptr_t)pl.cb < (uintptr_t)pl.cr ? pl.cb : pl.cr, 2 * cw, ch, (size_t)pl.c_stride, pl.c_frame_stride};
        return 2;
    }
    sp[1] = Span{pl.cb, cw, ch, (size_t)pl.c_stride, pl.c_frame_stride};
    sp[2] = Span{pl.cr, cw, ch, (size_t)pl.c_stride, pl.c_frame_stride};
    return 3;
}
int stage_planes(PlaneSet& ps, const vs_ycbcr_planes& pl, int n, int w, int h, size_t esz, int mem, bool out, hipStream_t s) {
    ps.dev = pl;
    if (mem == VS_MEM_DEVICE) return VS_OK;
    Span sp[3];
    const int k = spans_of(pl, w, h, sp);
    Staged* const st[3] = {&ps.y, &ps.c, &ps.c2};
    for (int i = 0; i < k; i++) {
        if (out) VS_TRY(st[i]->out_image(sp[i].p, sp[i].row_elems * esz, sp[i].rows, sp[i].stride * esz, (size_t)n, sp[i].fs * esz, mem));
        else VS_TRY(st[i]->in(sp[i].p, span_bytes(sp[i], n, esz), mem, s));
    }
    ps.dev.y = ps.y.dev;
    if (k == 2) {                                          // an interleaved pair: both pointers into the one span
        ps.dev.cb = (char*)ps.c.dev + ((char*)pl.cb - (char*)sp[1].p);
        ps.dev.cr = (char*)ps.c.dev + ((char*)pl.cr - (char*)sp[1].p);
    } else if (k == 3) { ps.dev.cb = ps.c.dev; ps.dev.cr = ps.c2.dev; }
    return VS_OK;
}

// what both calls and the stabilizer's wrapper ask of a descriptor and of the frame size; fn: the entry point an error names
int ycbcr_args_ok(const char* fn, const vs_ycbcr_planes* pl, int n, int w, int h, int format) {
    VS_ARG_AS(pl && n >= 1 && w > 0 && h > 0 && w <= 65535 && h <= 65535, fn);
    VS_TRY(bgr_format_ok(format));
    if (w > 32767 || h > 32767) return set_error(VS_ERR_UNSUPPORTED, "YCbCr conversion: frames up to 32767 x 32767, as the remap (%s)", fn);
    VS_ARG_AS(vsy::layout_ok(*pl, n, w, h), fn);
    const ptrdiff_t esz = vs_format_bits(format) > 8 ? 2 : 1;
    VS_ARG_AS(!pl->cb || pl->c_step == 1 || (char*)pl->cr - (char*)pl->cb == esz || (char*)pl->cb - (char*)pl->cr == esz, fn);
    return VS_OK;
}
int mem_ok(const char* fn, int mem) {
    VS_ARG_AS(mem == VS_MEM_HOST || mem == VS_MEM_DEVICE, fn);
    return VS_OK;
}
vs_ycbcr_planes at_frame(vs_ycbcr_planes pl, size_t f0, size_t esz) {
    pl.y = (char*)pl.y + f0 * pl.y_frame_stride * esz;
    if (pl.cb) { pl.cb = (char*)pl.cb + f0 * pl.c_frame_stride * esz; pl.cr = (char*)pl.cr + f0 * pl.c_frame_stride * esz; }
    return pl;
}

// planes (wherever `mem` says) -> BGR frames in device memory, on `s`.  Host planes: synchronises, the staged spans are released on return.
int planes_to_device_bgr(const vs_ycbcr_planes& src, int mem, int n, int w, int h, int format, void* bgr, size_t bgr_fs, int bgr_stride, hipStream_t s) {
    const size_t esz = vs_format_bits(format) > 8 ? 2 : 1;
    PlaneSet in;
    VS_TRY(stage_planes(in, src, n, w, h, esz, mem, false, s));
    VS_HIP(vsk::ycbcr_to_bgr(in.dev, n, w, h, vs_format_bits(format), vs_format_max_value(format), bgr, bgr_fs, bgr_stride, s));
    if (mem == VS_MEM_HOST) { VS_HIP(hipStreamSynchronize(s)); host_synced(); }
    return VS_OK;
}
// BGR frames in device memory -> planes (wherever `mem` says), on `s`.  Host planes: synchronises and copies the rows' own samples back.
int device_bgr_to_planes(const void* bgr, size_t bgr_fs, int n, int w, int h, int bgr_stride, int format, const vs_ycbcr_planes& dst, int mem, hipStream_t s) {
    const size_t esz = vs_format_bits(format) > 8 ? 2 : 1;
    PlaneSet out;
    VS_TRY(stage_planes(out, dst, n, w, h, esz, mem, true, s));
    VS_HIP(vsk::bgr_to_ycbcr(bgr, bgr_fs, n, w, h, bgr_stride, vs_format_bits(format), vs_format_max_value(format), out.dev, s));
    return finish_outputs(mem, s, {&out.y, &out.c, &out.c2});
}

}  // namespace

extern "C" {

int vs_ycbcr_to_bgr_batch(const vs_ycbcr_planes* src, int n, int w, int h, int format, void* dst, size_t dst_fs, int dst_stride, int mem, void* stream) try {
    VS_TRY(ycbcr_args_ok(__func__, src, n, w, h, format));
    VS_TRY(mem_ok(__func__, mem));
    const plan::Batch out{dst, dst_fs, n, w, h, dst_stride, 3, vs_format_bits(format)};
    VS_ARG(dst && out.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    PlaneSet in;
    Staged o;
    VS_TRY(stage_planes(in, *src, n, w, h, out.esz(), mem, false, s));
    VS_TRY(stage_out(o, out, mem, out.esz()));
    VS_HIP(vsk::ycbcr_to_bgr(in.dev, n, w, h, vs_format_bits(format), vs_format_max_value(format), o.dev, dst_fs, dst_stride, s));
    return finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_bgr_to_ycbcr_batch(const void* src, size_t src_fs, int n, int w, int h, int src_stride, int format, const vs_ycbcr_planes* dst, int mem, void* stream) try {
    VS_TRY(ycbcr_args_ok(__func__, dst, n, w, h, format));
    VS_TRY(mem_ok(__func__, mem));
    const plan::Batch in{src, src_fs, n, w, h, src_stride, 3, vs_format_bits(format)};
    VS_ARG(src && in.strides_ok());
    if (!device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a;
    VS_TRY(stage_in(a, in, mem, s));
    return device_bgr_to_planes(a.dev, src_fs, n, w, h, src_stride, format, *dst, mem, s);
} VS_CATCH_ALL

int vs_stabilizer_process_batch_ycbcr(vs_stabilizer* s, const vs_ycbcr_planes* frames, int n, int w, int h, int format, int mem, const vs_ycbcr_planes* out,
                                      int32_t* has_output, int* out_w, int* out_h) try {
    VS_ARG(s && frames && out && has_output && out_w && out_h);
    VS_TRY(ycbcr_args_ok(__func__, frames, n, w, h, format));
    VS_TRY(mem_ok(__func__, mem));
    const int crop = stab_crop(s);
    VS_ARG(w > 2 * crop && h > 2 * crop);
    int ow = 0, oh = 0;                                    // the delivered size: the crop window, or the handle's output size
    stab_delivered_size(s, w, h, &ow, &oh);
    VS_ARG(ow >= 1 && oh >= 1);
    VS_TRY(ycbcr_args_ok(__func__, out, n, ow, oh, format));
    if (!device_ready()) return VS_ERR_HIP;
    VS_HIP(hipSetDevice(stab_device(s)));
    hipStream_t st = (hipStream_t)vs_stabilizer_stream(s);
    const size_t esz = vs_format_bits(format) > 8 ? 2 : 1, in_fs = (size_t)w * h * 3, out_fs = (size_t)ow * oh * 3;
    // the two BGR buffers the handle keeps for this entry point: the converted input batch and the inner call's outputs
    YcbcrHold* const hold = stab_ycbcr_hold(s);
    VS_HIP(grow(&hold->buf[0], &hold->bytes[0], (size_t)n * in_fs * esz, st, true));
    VS_HIP(grow(&hold->buf[1], &hold->bytes[1], (size_t)n * out_fs * esz, st, true));
    // (a failure up to here, or of the conversion, leaves the stabilizer's state as it was)
    VS_TRY(planes_to_device_bgr(*frames, mem, n, w, h, format, hold->buf[0], in_fs, 3 * w, st));
    const int r = vs_stabilizer_process_batch(s, hold->buf[0], in_fs, n, w, h, 3 * w, format, VS_MEM_DEVICE, hold->buf[1], out_fs, has_output, out_w, out_h);
    if (r < 0) return r;                                   // (the inner call's failure protocol has run)
    // every contiguous run of output frames back into the caller's planes, index for index
    const int back = guarded([&] {
        for (int i = 0; i < n;) {
            if (!has_output[i]) { i++; continue; }
            int j = i + 1;
            while (j < n && has_output[j]) j++;
            VS_TRY(device_bgr_to_planes((const char*)hold->buf[1] + (size_t)i * out_fs * esz, out_fs, j - i, ow, oh, 3 * ow, format, at_frame(*out, (size_t)i, esz), mem, st));
            i = j;
        }
        return VS_OK;
    });
    if (back != VS_OK) {                                   // the engine calls' protocol: the running sequence ends, the handle stays usable
        const std::string why = vs_last_error();
        (void)hipStreamSynchronize(st);
        (void)vs_stabilizer_reset(s);
        return set_error(back, "%s", why.c_str());
    }
    return r;
} VS_CATCH_ALL

}  // extern "C"
