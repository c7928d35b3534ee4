// vs_capi.hip -- the stage kernels' entry points of the C ABI (include/vs_amd.h), with the debug and test entry points.
// Each mirrors one Halide AOT function the reference's imgproc.cpp calls; see the header for the
// file:line of the interface it replaces.  VS_MEM_HOST stages through device memory and syncs;
// VS_MEM_DEVICE only enqueues on the caller's stream.  (The frame warp and the border fill: vs_capi_warp.hip; the other look-ahead passes:
// vs_capi_lookahead.hip; staging, allocation and the rings behind all of them: vs_runtime.hip.)
#include "vs_capi.hpp"
#include "vs_phase.hpp"

#include <algorithm>
#include <cstdio>

using vsi::Staged;
using vsi::set_error;
using vsi::plan::img_span;

// ---- the debug build's bounds record (vs_device.hpp, -DVS_DEBUG_BOUNDS) ---------------------------------------------------
#ifdef VS_DEBUG_BOUNDS
#include "vs_device.hpp"
extern "C" int vs_bounds_fetch_engine(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_warp(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_phase(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_flow(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_fill(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_inpaint(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_deblur(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_denoise(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_deflicker(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_scene(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_fidelity(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_sharpen(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_rolling(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_remap(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_ycbcr(unsigned out[8], int reset);
extern "C" int vs_bounds_fetch_resize(unsigned out[8], int reset);
VS_BOUNDS_TU(vs_bounds_fetch_capi)
namespace {
// the checker checked: element 11 of an 8-element LDS array through a Span -- reported under site 900, executed on element 0
__global__ void vs_k_bounds_selftest(int* out) {
    __shared__ int arr[8];
    if (threadIdx.x < 8) arr[threadIdx.x] = 100 + (int)threadIdx.x;
    __syncthreads();
    VS_SPAN(int*, a, arr, 8, 900);
    if (threadIdx.x == 3) out[0] = a[11] + a[2];          // 100 (element 0 stands in) + 102
}
// every translation unit with instrumented kernels: where its record is fetched, and the name a report gives it
const struct { int (*fetch)(unsigned*, int); const char* name; } kBoundsUnits[] = {
    {vs_bounds_fetch_engine, "vs_engine.hip"}, {vs_bounds_fetch_warp, "vs_warp.hip"}, {vs_bounds_fetch_phase, "vs_phase.hip"}, {vs_bounds_fetch_flow, "vs_flow.hip"},
    {vs_bounds_fetch_fill, "vs_fill.hip"}, {vs_bounds_fetch_deblur, "vs_deblur.hip"}, {vs_bounds_fetch_denoise, "vs_denoise.hip"},
    {vs_bounds_fetch_deflicker, "vs_deflicker.hip"}, {vs_bounds_fetch_scene, "vs_scene.hip"}, {vs_bounds_fetch_fidelity, "vs_fidelity.hip"}, {vs_bounds_fetch_sharpen, "vs_sharpen.hip"}, {vs_bounds_fetch_rolling, "vs_rolling.hip"}, {vs_bounds_fetch_remap, "vs_remap.hip"}, {vs_bounds_fetch_ycbcr, "vs_ycbcr.hip"}, {vs_bounds_fetch_resize, "vs_resize.hip"}, {vs_bounds_fetch_inpaint, "vs_inpaint.hip"}, {vs_bounds_fetch_capi, "vs_capi.hip"}};
}  // namespace
#endif

extern "C" {

int vs_stream_retire(void* stream) try {
    VS_HIP(vsi::retire_stream((hipStream_t)stream));      // a fault of the work that was in flight on the stream surfaces here
    return VS_OK;
} VS_CATCH_ALL

int vs_debug_bounds_check(void) try {
#ifdef VS_DEBUG_BOUNDS
    if (!vsi::device_ready()) return VS_ERR_HIP;
    VS_HIP(hipDeviceSynchronize());
    unsigned total = 0;
    char msg[512] = "";
    for (const auto& u : kBoundsUnits) {
        unsigned r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (u.fetch(r, 1) != 0) return set_error(VS_ERR_HIP, "bounds record of %s is not readable", u.name);
        if (r[0] && !total)
            snprintf(msg, sizeof msg, "%s: site %u, index %d, limit %u, workgroup %u, thread %u", u.name, r[1], (int)r[2], r[3], r[4], r[5]);
        total += r[0];
    }
    if (total) set_error(VS_ERR_STATE, "%u out-of-bounds index(es) since the last check; first: %s", total, msg);
    return (int)std::min<unsigned>(total, 0x7fffffffu);
#else
    return set_error(VS_ERR_UNSUPPORTED, "vs_debug_bounds_check: this is not a -DVS_DEBUG_BOUNDS build of libvs_amd (tools/build_variant.sh bounds)");
#endif
} VS_CATCH_ALL

int vs_debug_bounds_selftest(void) try {
#ifdef VS_DEBUG_BOUNDS
    if (!vsi::device_ready()) return VS_ERR_HIP;
    vsi::DevBuf out;
    VS_HIP(out.alloc(sizeof(int)));
    hipLaunchKernelGGL(vs_k_bounds_selftest, dim3(1), dim3(64), 0, nullptr, out.as<int>());
    VS_HIP(hipGetLastError());
    int v = 0;
    VS_HIP(hipMemcpy(&v, out.p, sizeof(int), hipMemcpyDeviceToHost));
    return v;                                  // 202 when the violating access was redirected to element 0
#else
    return set_error(VS_ERR_UNSUPPORTED, "vs_debug_bounds_selftest: this is not a -DVS_DEBUG_BOUNDS build of libvs_amd");
#endif
} VS_CATCH_ALL

int vs_test_fail_alloc(int k) try {
    return vsi::test_fail_alloc(k);
} VS_CATCH_ALL

int vs_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} VS_CATCH_ALL

int vs_calib_copy12(const void* src_dev, void* dst_dev, size_t bytes, void* stream) try {
    VS_ARG(src_dev && dst_dev && bytes >= 12);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    VS_HIP(vsk::calib_copy12(src_dev, dst_dev, bytes, (hipStream_t)stream));
    return VS_OK;
} VS_CATCH_ALL

// the shader clock from inside a kernel: s_memtime counts shader cycles, s_memrealtime a constant 100 MHz
__global__ __launch_bounds__(256) void vs_k_clock_probe(unsigned long long* out, float seed, int iters) {
    float a0 = seed + (float)threadIdx.x, a1 = a0 + 1.0f, a2 = a0 + 2.0f, a3 = a0 + 3.0f;
    const float m = 0.999999f, c = 1.0e-7f;
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_sched_barrier(0);
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            a0 = __builtin_fmaf(a0, m, c); a1 = __builtin_fmaf(a1, m, c); a2 = __builtin_fmaf(a2, m, c); a3 = __builtin_fmaf(a3, m, c);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned long long t1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
    if (blockIdx.x == 0 && threadIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
    if (a0 + a1 + a2 + a3 == 12345.678f) out[2] = 1;                  // keeps the chains alive
}

int vs_shader_clock_probe(void* stream, double* shader_mhz) try {
    VS_ARG(shader_mhz);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* d = nullptr;
    VS_HIP(vsi::dev_alloc((void**)&d, 4 * sizeof(unsigned long long)));
    unsigned long long h[2] = {0, 0};
    hipError_t e = hipMemsetAsync(d, 0, 4 * sizeof(unsigned long long), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(vs_k_clock_probe, dim3(2048), dim3(256), 0, s, d, 1.0f, 3000);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    VS_HIP(e);
    *shader_mhz = h[1] ? 100.0 * (double)h[0] / (double)h[1] : 0.0;
    return VS_OK;
} VS_CATCH_ALL

int vs_pyr_down(const uint8_t* in, int w, int h, int in_stride, uint8_t* out, int ow, int oh, int out_stride, int mem,
                void* stream) try {
    VS_DIMS(w, h); VS_DIMS(ow, oh);
    VS_ARG(in && out && w > 0 && h > 0 && ow > 0 && oh > 0 && in_stride >= w && out_stride >= ow);
    VS_ARG(2 * ow <= w + 1 && 2 * oh <= h + 1);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, b;
    VS_TRY(a.in(in, img_span(w, h, in_stride, 1), mem, s));
    VS_TRY(b.out_image(out, (size_t)ow, (size_t)oh, (size_t)out_stride, 1, 0, mem));
    VS_HIP(vsk::pyr_down(a.as<uint8_t>(), w, h, in_stride, b.as<uint8_t>(), ow, oh, out_stride, 1, 0, 0, s));
    return vsi::finish_outputs(mem, s, {&b});
} VS_CATCH_ALL

int vs_optimal_dft_size(int n) { return vsp::optimal_dft_size(n); }

int vs_phase_correlate(const uint8_t* a, const uint8_t* b, int w, int h, int stride, int mem, void* stream, float* surface,
                       double* result) try {
    VS_DIMS(w, h);
    VS_ARG(a && b && result && w > 0 && h > 0 && stride >= w);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    vsp::Context ctx;
    struct Guard { vsp::Context& c; ~Guard() { c.destroy(); } } guard{ctx};
    if (ctx.configure(w, h, s) != hipSuccess)
        return set_error(VS_ERR_UNSUPPORTED, "phase correlation: padded extent over %d (%dx%d image)", vsp::kMaxLine, w, h);
    Staged ia, ib, surf;
    VS_TRY(ia.in(a, img_span(w, h, stride, 1), mem, s));
    VS_TRY(ib.in(b, img_span(w, h, stride, 1), mem, s));
    vsi::DevBuf spec, G, surf_own, pairs, res;
    VS_HIP(spec.alloc(2 * ctx.spec_frame() * sizeof(float2)));
    VS_HIP(G.alloc(ctx.spec_frame() * sizeof(float2)));
    VS_HIP(pairs.alloc(sizeof(vsp::Pair)));
    VS_HIP(res.alloc(sizeof(vsp::Result)));
    float* d_surf;
    if (surface) { VS_TRY(surf.out(surface, ctx.surface_elems() * sizeof(float), mem)); d_surf = surf.as<float>(); }
    else { VS_HIP(surf_own.alloc(ctx.surface_elems() * sizeof(float))); d_surf = surf_own.as<float>(); }
    const vsp::Pair pr{0, 1};
    VS_HIP(hipMemcpyAsync(pairs.p, &pr, sizeof pr, hipMemcpyHostToDevice, s));
    VS_HIP(ctx.spectra(ia.as<uint8_t>(), 0, stride, 1, spec.as<float2>(), s));
    VS_HIP(ctx.spectra(ib.as<uint8_t>(), 0, stride, 1, spec.as<float2>() + ctx.spec_frame(), s));
    VS_HIP(ctx.correlate(spec.as<float2>(), pairs.as<vsp::Pair>(), 1, G.as<float2>(), d_surf, res.as<vsp::Result>(), s));
    if (surface) VS_TRY(surf.finish(s));
    vsp::Result r;
    VS_HIP(hipMemcpyAsync(&r, res.p, sizeof r, hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));        // the result is a host value: this call always synchronises
    vsi::host_synced();
    surf.complete();
    result[0] = r.dx; result[1] = r.dy; result[2] = r.response;
    return VS_OK;
} VS_CATCH_ALL

int vs_grad_xy(const uint8_t* in, int w, int h, int stride, float* gx, float* gy, int mem, void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(in && gx && gy && w > 0 && h > 0 && stride >= w);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, x, y;
    VS_TRY(a.in(in, img_span(w, h, stride, 1), mem, s));
    VS_TRY(x.out(gx, (size_t)w * h * 4, mem));
    VS_TRY(y.out(gy, (size_t)w * h * 4, mem));
    VS_HIP(vsk::grad_xy(a.as<uint8_t>(), w, h, stride, x.as<float>(), y.as<float>(), s));
    return vsi::finish_outputs(mem, s, {&x, &y});
} VS_CATCH_ALL

int vs_grad_argmax(const float* gx, const float* gy, int w, int h, int ts, uint16_t* lmx, uint16_t* lmy, int mem,
                   void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(gx && gy && lmx && lmy && w > 0 && h > 0 && ts >= 1 && ts <= 64);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t nt = (size_t)(w / ts) * (h / ts);
    Staged a, b, x, y;
    VS_TRY(a.in(gx, (size_t)w * h * 4, mem, s));
    VS_TRY(b.in(gy, (size_t)w * h * 4, mem, s));
    VS_TRY(x.out(lmx, nt * 2 * 2, mem));
    VS_TRY(y.out(lmy, nt * 2 * 2, mem));
    VS_HIP(vsk::grad_argmax(a.as<float>(), b.as<float>(), w, h, ts, x.as<uint16_t>(), y.as<uint16_t>(), s));
    return vsi::finish_outputs(mem, s, {&x, &y});
} VS_CATCH_ALL

int vs_sparse_jac(const float* gx, const float* gy, int w, int h, const uint16_t* lmx, const uint16_t* lmy, int tx, int ty,
                  float* out_x, float* out_y, int mem, void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(gx && gy && lmx && lmy && out_x && out_y && w > 0 && h > 0 && tx > 0 && ty > 0);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t nt = (size_t)tx * ty;
    Staged a, b, c, d, x, y;
    VS_TRY(a.in(gx, (size_t)w * h * 4, mem, s));
    VS_TRY(b.in(gy, (size_t)w * h * 4, mem, s));
    VS_TRY(c.in(lmx, nt * 4, mem, s));
    VS_TRY(d.in(lmy, nt * 4, mem, s));
    VS_TRY(x.out(out_x, nt * 16, mem));
    VS_TRY(y.out(out_y, nt * 16, mem));
    VS_HIP(vsk::sparse_jac(a.as<float>(), b.as<float>(), w, h, c.as<uint16_t>(), d.as<uint16_t>(), (int)nt, x.as<float>(),
                           y.as<float>(), s));
    return vsi::finish_outputs(mem, s, {&x, &y});
} VS_CATCH_ALL

int vs_keyframe_fused(const uint8_t* in, int w, int h, int stride, int ts, uint16_t* lmx, uint16_t* lmy, float* jx,
                      float* jy, int mem, void* stream) try {
    VS_ARG(in && lmx && lmy && jx && jy && w > 0 && h > 0 && stride >= w && ts >= 1 && ts <= 64);
    VS_ARG(w <= 65535 && h <= 65535);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t nt = (size_t)(w / ts) * (h / ts);
    Staged a, x, y, p, q;
    VS_TRY(a.in(in, img_span(w, h, stride, 1), mem, s));
    VS_TRY(x.out(lmx, nt * 4, mem));
    VS_TRY(y.out(lmy, nt * 4, mem));
    VS_TRY(p.out(jx, nt * 16, mem));
    VS_TRY(q.out(jy, nt * 16, mem));
    VS_HIP(vsk::keyframe(a.as<uint8_t>(), w, h, stride, ts, x.as<uint16_t>(), y.as<uint16_t>(), p.as<float>(),
                         q.as<float>(), 1, 0, 0, 0, s));
    return vsi::finish_outputs(mem, s, {&x, &y, &p, &q});
} VS_CATCH_ALL

int vs_sparse_warpdiff(const uint8_t* tmpl, const uint8_t* key, int w, int h, int stride, const uint16_t* lm, int tx,
                       int ty, float A, float B, float TX, float TY, uint16_t* out, int mem, void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(tmpl && key && lm && out && w > 0 && h > 0 && stride >= w && tx > 0 && ty > 0);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    const size_t nt = (size_t)tx * ty;
    Staged a, b, c, o;
    VS_TRY(a.in(tmpl, img_span(w, h, stride, 1), mem, s));
    VS_TRY(b.in(key, img_span(w, h, stride, 1), mem, s));
    VS_TRY(c.in(lm, nt * 4, mem, s));
    VS_TRY(o.out(out, nt * 2, mem));
    VS_HIP(vsk::sparse_warpdiff(a.as<uint8_t>(), b.as<uint8_t>(), w, h, stride, c.as<uint16_t>(), (int)nt, A, B, TX, TY,
                                o.as<uint16_t>(), s));
    return vsi::finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_sparse_ica(const uint8_t* tmpl, const uint8_t* key, int w, int h, int stride, const uint16_t* selx, int nx,
                  const uint16_t* sely, int ny, const float* jacx, const float* jacy, float A, float B, float TX, float TY,
                  double* out4, int mem, void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(tmpl && key && out4 && w > 0 && h > 0 && stride >= w && nx >= 0 && ny >= 0);
    VS_ARG((nx == 0 || (selx && jacx)) && (ny == 0 || (sely && jacy)));
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, b, sx, sy, jx, jy, o;
    VS_TRY(a.in(tmpl, img_span(w, h, stride, 1), mem, s));
    VS_TRY(b.in(key, img_span(w, h, stride, 1), mem, s));
    VS_TRY(sx.in(selx, (size_t)nx * 4, mem, s));
    VS_TRY(sy.in(sely, (size_t)ny * 4, mem, s));
    VS_TRY(jx.in(jacx, (size_t)nx * 16, mem, s));
    VS_TRY(jy.in(jacy, (size_t)ny * 16, mem, s));
    VS_TRY(o.out(out4, 32, mem));
    VS_HIP(vsk::sparse_ica(a.as<uint8_t>(), b.as<uint8_t>(), w, h, stride, sx.as<uint16_t>(), nx, sy.as<uint16_t>(), ny,
                           jx.as<float>(), jy.as<float>(), A, B, TX, TY, o.as<double>(), s));
    return vsi::finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

int vs_image_warp(const uint8_t* in, int w, int h, int stride, float A, float B, float TX, float TY, float* out, int ow,
                  int oh, int mem, void* stream) try {
    VS_DIMS(w, h); VS_DIMS(ow, oh);
    VS_ARG(in && out && w > 0 && h > 0 && stride >= w && ow > 0 && oh > 0);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(a.in(in, img_span(w, h, stride, 1), mem, s));
    VS_TRY(o.out(out, (size_t)ow * oh * 4, mem));
    VS_HIP(vsk::image_warp(a.as<uint8_t>(), w, h, stride, A, B, TX, TY, o.as<float>(), ow, oh, s));
    return vsi::finish_outputs(mem, s, {&o});
} VS_CATCH_ALL
int vs_bgr_to_gray(const void* src, int w, int h, int src_stride, int bits, int shift_to_8, uint8_t* dst, int dst_stride,
                   int mem, void* stream) try {
    VS_DIMS(w, h);
    VS_ARG(src && dst && w > 0 && h > 0 && src_stride >= 3 * w && dst_stride >= w && (bits == 8 || bits == 16));
    VS_ARG(shift_to_8 >= 0 && shift_to_8 <= 8);
    if (!vsi::device_ready()) return VS_ERR_HIP;
    hipStream_t s = (hipStream_t)stream;
    Staged a, o;
    VS_TRY(a.in(src, img_span(w, h, src_stride, 3) * (bits / 8), mem, s));
    VS_TRY(o.out_image(dst, (size_t)w, (size_t)h, (size_t)dst_stride, 1, 0, mem));
    VS_HIP(vsk::bgr_to_gray(a.dev, w, h, src_stride, bits, shift_to_8, o.as<uint8_t>(), dst_stride, 1, 0, 0, s));
    return vsi::finish_outputs(mem, s, {&o});
} VS_CATCH_ALL

}  // extern "C"
