/*
 * vs_amd.h -- C ABI of libvs_amd.so: the MI355X (gfx950) alignment + warp engine.
 *
 * This is the drop-in boundary for the catid/video_stabilizer hot path.  Each entry point
 * names the reference interface it replaces (paths under the reference checkout).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Return: 0 = ok (or a documented positive value),
 *     negative = error; vs_last_error() returns a thread-local message.  No exceptions cross.
 *   - `mem` says where the caller's buffers live: VS_MEM_HOST (the library stages them through
 *     a pooled pinned mirror + device memory and synchronises: any alignment and pitch, pageable
 *     memory is fine; used by parity tests and one-off calls) or VS_MEM_DEVICE
 *     (device pointers; the call only enqueues work on `stream` and returns -- no sync).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - Images are row-major; strides are in ELEMENTS.  "planar (tx,ty,c)" tables are laid out
 *     like the reference's Halide buffers: element (x,y,c) at c*tx*ty + y*tx + x.
 *   - The caller owns every buffer it passes.  Handles own their device memory and one HIP
 *     stream; a handle is single-threaded, distinct handles are independent.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry point fails.
 */
#ifndef VS_AMD_H
#define VS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VS_OK 0
#define VS_ERR_ARG (-1)
#define VS_ERR_HIP (-2)
#define VS_ERR_UNSUPPORTED (-3)
#define VS_ERR_STATE (-4)
#define VS_ERR_NOMEM (-5)        /* a host allocation failed (std::bad_alloc), or another C++ exception was stopped at this boundary: the call is
                                   abandoned under the error protocol of its family (engine calls: the running sequence ends, the handle stays usable) */

enum { VS_MEM_HOST = 0, VS_MEM_DEVICE = 1 };
/* Frame formats.  16-bit containers say how many bits the samples really use: the aligner derives its 8-bit luma with
 * gray >> (bits - 8) and the stabilizer's warp saturates at vs_format_max_value().  The reference itself is 8-bit only
 * (imgproc.cpp:207-209); BASELINE config 5 ("4K 10-bit BGR") is VS_FMT_BGR10.
 * (ABI 5 retired VS_FMT_BGR16 = 5, the first release's "10-bit luma, 65535 saturation" format: value 5 is an unknown format now --
 * declare the depth the samples really have.) */
enum { VS_FMT_GRAY8 = 0, VS_FMT_BGR8 = 1, VS_FMT_BGR10 = 2, VS_FMT_BGR12 = 3, VS_FMT_BGR16_FULL = 4 };
/* bits per sample the alignment luma assumes: 8, 10, 12 or 16; 0 for an unknown format */
int vs_format_bits(int format);
/* largest sample value the stabilizer's warp stores: 255, 1023, 4095, 65535; 0 for an unknown format */
int vs_format_max_value(int format);
/* VS_WARP_LANCZOS2: the reference sampler's sequence of fp32 roundings with no contraction (bit-identical to the CPU
 * restatement's VSO_WARP_LANCZOS2).
 * VS_WARP_LANCZOS2_FAST: opt-in, the CONTRACTED form of the same sampler -- every Horner step and every tap accumulation a
 * single fma (what the reference's own target string, which carries `fma` and no strict_float, lets its compiler emit), the
 * tap order and the correctly rounded division unchanged; bit-identical to the CPU restatement's VSO_WARP_LANCZOS2_CONTRACTED
 * (np.array_equal, every layout), 1.27x faster at 4K.
 * VS_WARP_LANCZOS2_SEP: opt-in, the SEPARABLE form -- the contracted form's weights and taps, summed rows first, then columns,
 * over the product of the two 1-D weight sums, one correctly rounded reciprocal for all channels (equal to generators.cpp:687-697
 * in real arithmetic; a reassociation inside the reference's own non-strict_float slack).  Bit-identical to the CPU restatement's
 * VSO_WARP_LANCZOS2_SEPARABLE; against the UN-contracted order: at most 1 LSB, >= 99.99 % of the samples identical (8- and 10-bit;
 * SURVEY 8(d)'s integer gate, tests/test_warp_gate_gpu.py).
 * VS_WARP_BILINEAR_CV: cv::warpAffine(INTER_LINEAR) as the reference's stabilizer calls it (stabilizer.cpp:97-99 ->
 * imgproc.cpp:446-484): OpenCV 4.x's classic FIXED-POINT path -- the matrix inverted in double, source coordinates in 1/32 pixel
 * (AB_BITS 10, INTER_BITS 5), 15-bit integer weights, (sum + 2^14) >> 15 for 8-bit samples (float weights and cvRound for 16-bit
 * containers).  Integer work: bit-identical to the CPU restatement's VSO_WARP_BILINEAR_CV, no tolerance.  "Parity unpinned
 * (OpenCV version)": the reference installs libopencv-dev unpinned and OpenCV is not in this image; the restatement follows the
 * published 4.5 / 4.6 source.  IN THIS MODE `t` IS THE TRANSFORM HANDED TO warpBySimilarityTransform -- the FORWARD map, which
 * cv::warpAffine inverts itself (every other mode takes the sampling map); integer output only (no _f32 form). */
enum { VS_WARP_LANCZOS2 = 0, VS_WARP_BILINEAR = 1, VS_WARP_LANCZOS2_FAST = 2, VS_WARP_LANCZOS2_SEP = 3, VS_WARP_BILINEAR_CV = 4 };
enum { VS_BORDER_CLAMP = 0, VS_BORDER_CONSTANT = 1 };
/* how the per-level "keep the best 80 %" subset is chosen (alignment.cpp:460-486) */
enum {
    VS_SELECT_STL_HOST = 0,   /* D2H + the host's std::nth_element, literally as the reference */
    VS_SELECT_DEVICE = 1,     /* on-device replica of libstdc++'s introselect: same set, same order (the default) */
    VS_SELECT_STABLE = 2      /* on the device under a documented, STL-independent rule: the tiles that are
                               * smallest by (abs_delta, tile index) -- ties on abs_delta go to the lower tile index -- in ascending
                               * tile order.  A set any conforming std::nth_element may produce; the survivors' ORDER (which the
                               * reference leaves to its STL, and which the fp64 sums follow) is fixed, so the transforms differ
                               * from the other two modes in the last bits -- and beyond, where the tied tiles differ.  No partition
                               * rounds (a histogram finds the cut, ballots place the survivors): a quarter of the selection
                               * time, one AlignNextFrame call in 0.20 ms instead of 0.245 at 1080p (0.29 instead of 0.38 at 4K).
                               * Bit-identical to the oracle's vso_select_smallest_stable / select rule 1. */
};

/* imgproc.hpp:40-46 SimilarityTransform (centre-based, double) */
typedef struct vs_transform { double A, B, TX, TY; } vs_transform;
typedef struct vs_point { double x, y; } vs_point;

/* alignment.hpp:5-41 VideoAlignerParams -- same fields, same defaults */
typedef struct vs_aligner_params {
    int    phase_correlate;            /* alignment.hpp:11: start TX,TY from cv::phaseCorrelate on pyramid level 2 */
    double phase_correlate_threshold;
    double threshold;
    float  smallest_fraction;
    int    max_iters;
    int    pyramid_min_width;
    int    pyramid_min_height;
    double max_displacement;
} vs_aligner_params;

/* stabilizer.hpp:13-30 VideoStabilizerParams (+ the two warp knobs this build defines) */
typedef struct vs_stabilizer_params {
    vs_aligner_params aligner;
    int    lag;
    int    smoother_memory;
    double lambda;
    int    enable_smoother;
    int    crop_pixels;
    double min_disp, max_disp;
    double min_decay, max_decay;
    int    warp_mode;     /* VS_WARP_*   (reference: cv::warpAffine INTER_LINEAR, imgproc.cpp:472) */
    int    warp_border;   /* VS_BORDER_* (reference: BORDER_CONSTANT black, imgproc.cpp:479-480) */
} vs_stabilizer_params;

const char* vs_last_error(void);
const char* vs_version(void);
/* ABI number of the structs and enums in this header.  It changes whenever a struct grows, an enum value moves or a default changes its
 * meaning (4: vs_align_info carries selected_x / selected_y / level_transform; 5: VS_FMT_BGR16 retired, VS_WARP_LANCZOS2_SEP = 3 and
 * VS_WARP_BILINEAR_CV = 4 added, vs_stabilizer_params_default's warp_mode is VS_WARP_BILINEAR_CV).  The engine writes sizeof(vs_align_info) bytes per frame
 * into caller arrays, so a caller built against another header must not go on: check vs_abi_version() == VS_ABI_VERSION once
 * after loading the library (the facade classes do, and throw).  vs_sizeof_align_info() is the size the LIBRARY was built with. */
#define VS_ABI_VERSION 5
int    vs_abi_version(void);
size_t vs_sizeof_align_info(void);
/* number of usable HIP devices (0 when there is none; never fails) */
int vs_device_count(void);

void vs_aligner_params_default(vs_aligner_params* p);
void vs_stabilizer_params_default(vs_stabilizer_params* p);

/* ------------------------------------------------------------------------------------------
 * Host-side scalar algebra (no device needed)
 * ------------------------------------------------------------------------------------------ */
/* SimilarityTransform::inverse / compose / warp / maxCornerDisplacement, imgproc.cpp:333-437 */
vs_transform vs_transform_inverse(const vs_transform* t);
vs_transform vs_transform_compose(const vs_transform* t1, const vs_transform* t2);   /* t1 then t2 */
vs_point     vs_transform_warp(const vs_transform* t, vs_point p);
vs_point     vs_transform_warp_center(const vs_transform* t, vs_point p, double cx, double cy);
double       vs_transform_max_corner_displacement(const vs_transform* t, double width, double height);
/* GradArgMax's tile-size rule, imgproc.cpp:151-162 */
int vs_tile_size(int w, int h);
/* centre-based double transform -> the float, upper-left based kernel arguments.
 * sparse: imgproc.cpp:69-75 / 98-103 (centre w/2,h/2).  warp: imgproc.cpp:125-131 (centre (w-1)/2,(h-1)/2) */
void vs_ul_params_sparse(const vs_transform* t, int w, int h, float out4[4]);
void vs_ul_params_warp(const vs_transform* t, int w, int h, float out4[4]);
/* VS_WARP_BILINEAR_CV: the 2x3 matrix of warpBySimilarityTransform(t) for a w x h frame (imgproc.cpp:457-466), inverted the way
 * cv::warpAffine inverts a matrix given without WARP_INVERSE_MAP (double precision, OpenCV's operation order): row-major
 * {M0, M1, M2; M3, M4, M5}, the map from an output pixel to its source position. */
void vs_cv_inverse_matrix(const vs_transform* t, int w, int h, double out6[6]);
/* L1SmootherCenter, smoother.hpp:10-30 / smoother.cpp:67-127 */
typedef struct vs_smoother vs_smoother;
vs_smoother* vs_smoother_create(int lag_behind, int lag_ahead, double lambda);
void vs_smoother_destroy(vs_smoother* s);
int  vs_smoother_update(vs_smoother* s, const vs_transform* meas, vs_transform* out_finalized); /* 1 = finalized */
void vs_tvl1_smooth(const double* data, int n, double lambda, int iterations, double* out);   /* smoother.cpp:18-65 */

/* ------------------------------------------------------------------------------------------
 * Kernel level: one entry point per Halide AOT function called from imgproc.cpp
 * ------------------------------------------------------------------------------------------ */
/* int pyr_down(in, out)                                   imgproc.cpp:112, generators.cpp:56-92 */
int vs_pyr_down(const uint8_t* in, int w, int h, int in_stride,
                uint8_t* out, int ow, int oh, int out_stride, int mem, void* stream);
/* int grad_xy(in, gx, gy)                                 imgproc.cpp:140, generators.cpp:202-224
 * gx, gy dense (w*h) */
int vs_grad_xy(const uint8_t* in, int w, int h, int stride, float* gx, float* gy, int mem, void* stream);
/* int grad_argmax_<ts>(gx, gy, local_max_x, local_max_y)  imgproc.cpp:174-195, generators.cpp:260-294
 * tile_size 1..64; outputs planar (w/ts, h/ts, 2) u16 */
int vs_grad_argmax(const float* gx, const float* gy, int w, int h, int tile_size,
                   uint16_t* local_max_x, uint16_t* local_max_y, int mem, void* stream);
/* int sparse_jac(gx, gy, lmx, lmy, out_x, out_y)          imgproc.cpp:42, generators.cpp:332-386
 * outputs planar (tx,ty,4) f32 */
int vs_sparse_jac(const float* gx, const float* gy, int w, int h,
                  const uint16_t* local_max_x, const uint16_t* local_max_y, int tx, int ty,
                  float* out_x, float* out_y, int mem, void* stream);
/* Fused keyframe pass (what the engine runs): grad_xy + grad_argmax + sparse_jac straight from
 * the u8 image, never materialising the gradient planes.  Same outputs, bit for bit, as the
 * three calls above (alignment.cpp:237-276). */
int vs_keyframe_fused(const uint8_t* in, int w, int h, int stride, int tile_size,
                      uint16_t* local_max_x, uint16_t* local_max_y, float* jac_x, float* jac_y,
                      int mem, void* stream);
/* int sparse_warpdiff(tmpl, key, local_max, A, B, TX, TY, out)   imgproc.cpp:94-104, generators.cpp:646-700 */
int vs_sparse_warpdiff(const uint8_t* tmpl, const uint8_t* key, int w, int h, int stride,
                       const uint16_t* local_max, int tx, int ty,
                       float A, float B, float TX, float TY, uint16_t* out, int mem, void* stream);
/* int sparse_ica(tmpl, key, selx, sely, jacx, jacy, A, B, TX, TY, out)  imgproc.cpp:62-76, generators.cpp:429-596
 * selx/sely planar (n,2) u16; jacx/jacy planar (n,4) f32; out = 4 doubles */
int vs_sparse_ica(const uint8_t* tmpl, const uint8_t* key, int w, int h, int stride,
                  const uint16_t* selx, int nx, const uint16_t* sely, int ny,
                  const float* jacx, const float* jacy,
                  float A, float B, float TX, float TY, double* out4, int mem, void* stream);
/* The keep-best-fraction selection of alignment.cpp:435-492 as a device op, for n_arrays independent
 * warpdiff tables (each tx*ty u16, row-major): flatten, std::nth_element on abs_delta, keep the first
 * size_t(tx*ty*fraction).  out_idx: n_arrays x (tx*ty) int32, the first `count` of each row are the
 * surviving tile indices (tile_y*tx+tile_x) in the exact order libstdc++'s nth_element leaves them
 * (an on-device replica of its introselect).  status[a] = 1 if libstdc++ would have taken its
 * heap-select fallback for array a (not replicated; callers then use the host).  Returns count. */
int vs_select_smallest(const uint16_t* warpdiff, int n_arrays, int tx, int ty, float fraction,
                       int32_t* out_idx, int32_t* status, int mem, void* stream);
/* The same step under VS_SELECT_STABLE's rule: the first `count` entries of each row are the tiles that are
 * smallest by (abs_delta, tile index), in ascending tile order -- the oracle's vso_select_smallest_stable.  Returns count. */
int vs_select_smallest_stable(const uint16_t* warpdiff, int n_arrays, int tx, int ty, float fraction,
                              int32_t* out_idx, int mem, void* stream);
/* cv::phaseCorrelate(a, b, cv::noArray(), &response) as VideoAligner calls it (alignment.cpp:372-374) on the CV_32F copy
 * of pyramid level 2 (alignment.cpp:225-229): two w x h u8 images -> result[3] = {shift.x, shift.y, response} in host
 * memory (the call synchronises).  Images are zero-padded to vs_optimal_dft_size (cv::getOptimalDFTSize: 2^a 3^b 5^c);
 * surface: NULL, or M*N floats (M, N = padded h, w; in `mem`) receiving the unshifted, unscaled correlation surface.
 * OpenCV is not part of the reference tree: the transform specification is this build's (oracle/vs_phase.cpp). */
int vs_phase_correlate(const uint8_t* a, const uint8_t* b, int w, int h, int stride, int mem, void* stream, float* surface,
                       double* result);
int vs_optimal_dft_size(int n);
/* int image_warp(in, A, B, TX, TY, out)                   imgproc.cpp:131, generators.cpp:126-164 */
int vs_image_warp(const uint8_t* in, int w, int h, int stride,
                  float A, float B, float TX, float TY, float* out, int ow, int oh, int mem, void* stream);
/* Streams passed to the bgr_image_warp entry points: the library keeps one event per in-flight call on the caller's stream (its
 * parameter ring) until a later call on the same thread retires it.  Before DESTROYING such a stream call vs_stream_retire(stream):
 * it waits for the library's work on that stream and drops every reference to it.  (Handles do this for their own streams.) */
int vs_stream_retire(void* stream);
/* bgr_image_warp: the full-frame colour warp (replaces warpBySimilarityTransform's cv::warpAffine,
 * imgproc.cpp:446-484 / stabilizer.cpp:97-99; the generator itself is absent from the reference,
 * schedules/bgr_image_warp.schedule.h is its orphan -- SURVEY D2).  `t` is the output->input
 * sampling map, centre-based about ((w-1)/2,(h-1)/2) as ImageWarp (imgproc.cpp:125-131).
 * src/dst interleaved with `channels` (1..4) per pixel; bits 8 (uint8_t) or 16 (uint16_t);
 * store rule floor(v+0.5) saturated to [0,max_value].  n_frames >= 1 frames are processed in one
 * launch: frame i at src + i*src_frame_stride (elements), transform t[i]. */
int vs_bgr_image_warp(const void* src, int w, int h, int src_stride, int channels, int bits,
                      const vs_transform* t, int mode, int border, int max_value,
                      void* dst, int dst_stride, int mem, void* stream);
int vs_bgr_image_warp_batch(const void* src, size_t src_frame_stride, int n_frames,
                            int w, int h, int src_stride, int channels, int bits,
                            const vs_transform* t /* host array, n_frames */, int mode, int border, int max_value,
                            void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* The same, but only the window [roi_x, roi_x+roi_w) x [roi_y, roi_y+roi_h) of every output frame is computed and
 * stored (dst holds roi_w x roi_h pixels per frame, row stride dst_stride, frame stride dst_frame_stride): bit-identical
 * to cropping the full warp.  This is how the stabilizer applies crop_pixels (stabilizer.cpp:102-109) without warping the
 * margin or copying the frame. */
int vs_bgr_image_warp_roi_batch(const void* src, size_t src_frame_stride, int n_frames, int w, int h, int src_stride,
                                int channels, int bits, const vs_transform* t, int mode, int border, int max_value,
                                int roi_x, int roi_y, int roi_w, int roi_h,
                                void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* VS_WARP_BILINEAR_CV with BORDER FILL: what an output frame's own source does not cover is taken from other source frames.
 * 3 channels, 8- or 16-bit containers, both borders, frames up to 32767 x 32767 (VS_ERR_UNSUPPORTED beyond: cv::warpAffine
 * saturates source coordinates to short there).  Output frame o (n_out of them) has n_cand (1 .. 16) candidates c, each a
 * (source frame, forward transform) pair in VS_WARP_BILINEAR_CV's convention: frame cand_frame[o*n_cand + c] of the batch at
 * `src` (0 <= index < n_src; a negative index ends the list) and cand_t[o*n_cand + c].  Candidate 0 is the frame itself.
 *   - For a candidate with sampling matrix M (vs_cv_inverse_matrix of its transform) output pixel (x, y) -- full-frame
 *     coordinates, also under a ROI -- has the integer source position of the warp itself: X = (X0[y] + adelta[x]) >> 5,
 *     sx = X >> 5, X0[y] = cvRound((M[1] y + M[2]) 1024) + 16, adelta[x] = cvRound(M[0] x 1024); sy likewise from M[3 .. 5].
 *     int32 throughout, as in cv::warpAffine: cvRound saturates to [INT_MIN, INT_MAX] (NaN gives 0), and the additions (+ 16,
 *     X0 + adelta) wrap in two's complement before the arithmetic shifts.  An extreme matrix (a near-singular transform, a
 *     shift beyond 2^21 pixels) is therefore judged on the saturated, wrapped position -- the one the plain warp samples.
 *     The candidate COVERS the pixel iff all four taps lie in the frame: 0 <= sx, sx + 1 <= w - 1, 0 <= sy, sy + 1 <= h - 1.
 *   - The pixel's value is the value VS_WARP_BILINEAR_CV gives for the FIRST candidate that covers it, bit for bit.  If no
 *     candidate covers it, it keeps candidate 0's ordinary result under `border`.
 *   - Hence pixels candidate 0 covers are exactly the plain warp's, and n_cand == 1 is the roi_batch call above, bit for
 *     bit.  No blending, feathering or photometric matching in this call: see vs_bgr_image_warp_fill_blend_batch below.
 * ROI, strides, mem, stream: as in the roi_batch call; cand_frame and cand_t are host arrays of n_out * n_cand entries. */
int vs_bgr_image_warp_fill_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride,
                                 int channels, int bits, int n_out, int n_cand, const int32_t* cand_frame,
                                 const vs_transform* cand_t, int border, int max_value,
                                 int roi_x, int roi_y, int roi_w, int roi_h,
                                 void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* THE FILL WITH ITS SEAMS BLENDED: two independent switches on the fill above, both exact integer rules.  Candidates, coverage, the
 * int32 positions X, Y (5 fraction bits) and the sample q_c of a covering candidate are vs_bgr_image_warp_fill_batch's.
 *   - Channel sums: S_i,c = the sum of the raw samples of channel c over all w x h pixels of frame i, as uint64_t; no clamp to the
 *     format's maximum.  S <= 65535 * 32767^2 < 2^46; integer sums, so the order of the reduction cannot matter.
 *   - Gain (match == 1) of candidate j >= 1 for output frame k (candidate 0's frame), per channel c, Q15, unsigned 64-bit:
 *     G = 32768 if S_j,c == 0 or S_k,c == 0; otherwise G = clamp((2 * 32768 * S_k,c + S_j,c) / (2 * S_j,c), 16384, 65536) with
 *     floor division (every term below 2^63).  With match == 0, G = 32768.
 *   - Matched fill sample of the FIRST candidate j >= 1 that covers the pixel (q_c <= max_value):
 *     f_c = min((q_c * G + 16384) >> 15, max_value) in unsigned 32-bit (65535 * 65536 + 16384 < 2^32).
 *   - A pixel candidate 0 does not cover: out_c = f_c if a later candidate covers it; otherwise candidate 0's result under
 *     `border`, as in the fill.
 *   - Band pixel (feather >= 1): K = 32 << feather, Xmax = (w - 1) * 32 - 1, Ymax = (h - 1) * 32 - 1.  A pixel candidate 0 covers
 *     has 0 <= X <= Xmax and 0 <= Y <= Ymax; d = min(X, Xmax - X, Y, Ymax - Y), k = d + 1.  If k >= K, or no later candidate covers
 *     the pixel, it is the plain warp's value p_c bit for bit; otherwise
 *     out_c = (k * p_c + (K - k) * f_c + K / 2) >> (5 + feather)   (the sum is below 2^27: unsigned 32-bit).
 *   - Hence (a) feather == 0 && match == 0 is vs_bgr_image_warp_fill_batch bit for bit; (b) n_cand == 1, or a list whose later
 *     entries are all negative, is the plain ROI warp; (c) a band pixel lies between min(p_c, f_c) and max(p_c, f_c);
 *     (d) identical frames under identity maps come back bit for bit with any setting; (e) a pixel at least 2^feather source
 *     pixels inside candidate 0's frame is never changed.
 * feather: 0 (off) or 1 .. 6; match: 0 or 1; anything else is VS_ERR_ARG. */
typedef struct vs_fill_blend_params { int feather; int match; } vs_fill_blend_params;
/* sums[3*i + c] = S_i,c of frame i (n frames, frame i at src + i*src_frame_stride elements); every VS_FMT_BGR*, frames up to
 * 32767 x 32767 (VS_ERR_UNSUPPORTED beyond, as in the fill); `sums` lives in `mem`. */
int vs_bgr_channel_sums_batch(const void* src, size_t src_frame_stride, int n, int w, int h, int src_stride, int format,
                              uint64_t* sums, int mem, void* stream);
/* The fill call's arguments plus sums (3 * n_src values in `mem`, as vs_bgr_channel_sums_batch leaves them; NULL is allowed only
 * with match == 0) and params (required). */
int vs_bgr_image_warp_fill_blend_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride,
                                       int channels, int bits, int n_out, int n_cand, const int32_t* cand_frame,
                                       const vs_transform* cand_t, const uint64_t* sums, const vs_fill_blend_params* params,
                                       int border, int max_value, int roi_x, int roi_y, int roi_w, int roi_h,
                                       void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* DEBLUR BY TRANSFER: a frame that shake has blurred is blended with what its SHARPER neighbours show at the same scene point
 * (Matsushita et al. 2006; the role of OpenCV videostab's WeightingDeblurer).  Interleaved BGR, every VS_FMT_BGR*.  The rule:
 *   - Gray g = min(((B*3735 + G*19235 + R*9798 + 16384) >> 15) >> (bits - 8), 255): vs_bgr_to_gray's rule shifted to 8 bits.
 *   - Sharpness of a frame: S = sum over 1 <= x <= w-2, 1 <= y <= h-2 of (g(x+1,y) - g(x-1,y))^2 + (g(x,y+1) - g(x,y-1))^2 as
 *     uint64_t (integer sums: exact; S <= 130050 w h < 2^53, so (double)S is exact).
 *   - Output frame o has n_cand (1 .. 16) candidates c: frame cand_frame[o*n_cand + c] of the batch at `src` (a negative index
 *     ends the list) and cand_t[o*n_cand + c], exactly as in vs_bgr_image_warp_fill_batch.  Candidate 0 is the target frame k
 *     itself; its transform is ignored.  Candidate j takes part iff S_j > S_k, strictly, with
 *     r_j = (float)min((double)S_j / (double)max(S_k, 1), (double)max_ratio).  If no candidate takes part the frame is copied.
 *   - With M = vs_cv_inverse_matrix(cand_t) target pixel (x, y) lies in candidate j at qx = rint((M0 x + M1 y) + M2),
 *     qy = rint((M3 x + M4 y) + M5) (double, that order, no fma, ties to even): VS_WARP_BILINEAR_CV's convention and centre.
 *     Nearest sample.  Outside the frame the candidate contributes nothing at that pixel; otherwise, with
 *     d = |g_k(x,y) - g_j(qx,qy)| as float, w = (r_j * r_j) / (d + sensitivity) in fp32 with a correctly rounded division.  Per
 *     channel acc_c = p_c + sum_j w q_c and W = 1 + sum_j w, in candidate order, fp32, no fma; the output is
 *     floor(acc_c / W + 0.5) saturated to the format's maximum.
 *   - Hence a frame with no sharper candidate, identical frames (ties on S) and n_cand == 1 come back bit for bit.
 * sensitivity: gray levels (> 0); max_ratio (> 0) bounds r_j, so that a dark or flat frame (a fade) is not replaced by its
 * neighbour.  Accepted (VS_ERR_ARG otherwise): 0 < sensitivity <= 3e38, 0 < max_ratio <= 1e18 and, evaluated in double,
 * min(max_ratio, 2^53)^2 <= sensitivity * 2^100.  S < 2^53 bounds r_j by the same minimum, so a weight is at most 2^100 and the
 * fp32 sums of at most 15 weights times samples <= 65535 stay below 2^121: acc_c and W are finite for every frame, and the rule
 * defines every output sample.  (Outside it W reaches inf -- a black target, sensitivity 1e-38 -- and acc_c / W is inf / inf.) */
typedef struct vs_deblur_params { float sensitivity; float max_ratio; } vs_deblur_params;
void vs_deblur_params_default(vs_deblur_params* p);   /* 2, 4 */
/* sharpness[i] = S of frame i (n frames, frame i at src + i*src_frame_stride elements); `sharpness` lives in `mem` */
int vs_bgr_sharpness_batch(const void* src, size_t src_frame_stride, int n, int w, int h, int src_stride, int format,
                           uint64_t* sharpness, int mem, void* stream);
/* sharpness: the S of the n_src frames at `src` (in `mem`, as vs_bgr_sharpness_batch leaves them); cand_frame and cand_t are
 * host arrays of n_out * n_cand entries; dst holds full w x h frames.  VS_MEM_DEVICE only enqueues. */
int vs_bgr_deblur_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride, int format,
                        const uint64_t* sharpness, int n_out, int n_cand, const int32_t* cand_frame, const vs_transform* cand_t,
                        const vs_deblur_params* params /* NULL = defaults */,
                        void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* TEMPORAL DENOISE, MOTION COMPENSATED: a pixel is averaged with what other frames show at the same scene point, as far as they agree
 * with it.  Interleaved BGR, every VS_FMT_BGR*, frames up to 32767 x 32767 (VS_ERR_UNSUPPORTED beyond, as in the fill).  The rule:
 *   - Output frame o has n_cand (1 .. 16) candidates (cand_frame, cand_t), exactly as in vs_bgr_deblur_batch.  Candidate 0 is the target
 *     frame k itself and its transform is ignored; a negative index ends the list.
 *   - cand_t is in VS_WARP_BILINEAR_CV's forward convention.  The sample q_c of candidate j at target pixel (x, y) is, bit for bit, what
 *     vs_bgr_image_warp_roi_batch gives in mode VS_WARP_BILINEAR_CV for that frame and transform with max_value =
 *     vs_format_max_value(format): cv::warpAffine's fixed-point bilinear on int32 positions (see vs_bgr_image_warp_fill_batch).
 *     Candidate j takes part at the pixel only if it COVERS it by the fill's rule: all four taps at the warp's own integer source
 *     position lie in the frame.  No sample ever meets a border rule.
 *   - All arithmetic in unsigned 32-bit integers.  s = bits - 8; t = strength, 1 .. 255, in 8-bit levels (default 24).
 *       d_j = max over the three channels of |p_c - q_c| >> s;      w_j = t - d_j if d_j < t, else 0
 *       acc_c = t p_c + sum_j w_j q_c;      W = t + sum_j w_j
 *     If sum_j w_j == 0 the pixel is p_c, bit for bit.  Otherwise it is min((2 acc_c + W) / (2 W), max_value), floor division.
 *   - Bound: 2 acc_c + W <= 2 * 16 * 255 * 65535 + 4080 < 2^30, so every term fits and the rule defines every sample for every input
 *     the call accepts.
 *   - Hence (a) n_cand == 1, an all-negative list and candidates that lie wholly outside the frame give the frame back bit for bit;
 *     (b) identical frames under identity maps come back bit for bit; (c) |out_c - p_c| < t << s at every pixel, whatever the content
 *     and the maps (the ghost bound); (d) a pixel whose candidates all differ from it by t levels or more in some channel is untouched.
 * A strength outside 1 .. 255 is VS_ERR_ARG. */
typedef struct vs_denoise_params { int strength; } vs_denoise_params;
void vs_denoise_params_default(vs_denoise_params* p);   /* 24 */
/* cand_frame and cand_t are host arrays of n_out * n_cand entries; dst holds full w x h frames.  VS_MEM_DEVICE only enqueues.  The
 * candidate entries reach the device in groups of (kSlots / 2 / 4) / n_cand output frames (kSlots = 32768 slots of the parameter ring, an
 * entry is four slots: 256 frames at 16 candidates, 2048 at 2); a group whose targets or destination do not all start on dwords takes the
 * per-sample kernel, with the same result. */
int vs_bgr_denoise_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride, int format,
                         int n_out, int n_cand, const int32_t* cand_frame, const vs_transform* cand_t,
                         const vs_denoise_params* params /* NULL = defaults */,
                         void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* ROLLING-SHUTTER CORRECTION: a rolling-shutter sensor exposes a frame row by row, so camera motion shears and bends the frame from inside.
 * Every row is resampled to what a global shutter would have shown at the middle row's time, from the motion to the frame that follows.
 * THE RULE.
 * Interleaved BGR, every `VS_FMT_BGR*`, frames up to 32767 x 32767. Beyond that the call returns `VS_ERR_UNSUPPORTED`, as the denoise does.
 *
 * Inputs
 *
 * - Output frame `o` has exactly two candidate entries `(cand_frame, cand_t)`, laid out as in `vs_bgr_denoise_batch` with `n_cand == 2`.
 * - Entry 0 is the frame to correct. Its transform is ignored.
 * - Entry 1 carries the motion to the frame that follows it, in `VS_WARP_BILINEAR_CV`'s forward convention.
 * - For entry 1 only the sign of `cand_frame` is looked at. That frame's pixels are never read.
 * - A negative index means "no motion known".
 * - `M[0..5] = vs_cv_inverse_matrix(cand_t[1], w, h)` is where pixel `(x, y)` of the frame lies in the following frame.
 * - `readout` (`rho`) is the share of the frame period that the sensor takes to scan the frame from row 0 to row `h - 1`. Its range is
 *   -1 .. 1; negative values mean bottom-up scanning. NaN or a value outside the range is `VS_ERR_ARG`.
 *
 * Row time
 *
 * `tau(y) = rho * ((double)(2 * y - (h - 1)) / (double)(2 * h))`.
 *
 * It is zero at the frame's middle. Every product and sum rounds once, in the order written: the build's `-ffp-contract=off`, no explicit FMA.
 *
 * Row matrix (fp64, same order)
 *
 * - `r0 = 1 + tau * (M0 - 1)`, `r1 = tau * M1`, `r2 = tau * M2`
 * - `r3 = tau * M3`, `r4 = 1 + tau * (M4 - 1)`, `r5 = tau * M5`
 *
 * The row matrix is again of similarity form. The scene point that a global shutter would have shown at `(x, y)` sits in the raw frame at
 * `r(y) * (x, y, 1)`. This is first order in the intra-frame motion.
 *
 * Position
 *
 * The position rule is `VS_WARP_BILINEAR_CV`'s own int32 rule, with the row's matrix in place of the frame's.
 *
 * - `X = (cv_row_origin(r1, r2, y) + cv_delta(r0, x)) >> 5`, `Y` likewise from `r4, r5, r3`. This is `cv_pos` of `vs_device.hpp`.
 * - It keeps that rule's saturating `cvRound`, NaN -> 0, wrapping sums and arithmetic shifts.
 * - The position has 5 fraction bits.
 *
 * Sample
 *
 * The blend is `VS_WARP_BILINEAR_CV`'s blend of the four taps at `(X >> 5, Y >> 5)` with fractions `X & 31`, `Y & 31`.
 *
 * - 8-bit containers: integer weights, `(sum + 512) >> 10`.
 * - 16-bit containers: weights `a * b / 1024` in fp32, `rintf`, saturated to `vs_format_max_value(format)`.
 * - Border: each tap's column is clamped to `0 .. w - 1` and its row to `0 .. h - 1`. The weights are unchanged.
 * - No border colour can enter a corrected frame, so `warp_border` plays no part.
 *
 * Hence
 *
 * - (a) No motion: the frame comes back bit for bit, as a dword copy where the rows allow it.
 * - (b) `rho == 0`: bit for bit.
 * - (c) A motion of `{0, 0, 0, 0}`: bit for bit.
 * - (d) For odd `h`, row `(h - 1) / 2` comes back bit for bit whatever the motion.
 * - (e) Every output sample lies between the minimum and the maximum of the frame's samples in that channel.
 * - (f) The rule defines every sample for every input the call accepts: NaN, singular and saturating matrices included.
 * ((b) - (d): for samples up to the format's maximum and a finite motion -- the blend at zero fraction is the sample, which a 16-bit container
 * then saturates, and tau * NaN is NaN whatever tau.)
 * The default readout, 0.5, is a PLACEHOLDER in the middle of what phone and action-camera sensors do, not a measured sensor value: take the
 * figure from the sensor's data sheet (line time x rows / frame period) or calibrate it. */
typedef struct vs_rolling_params { double readout; } vs_rolling_params;
void vs_rolling_params_default(vs_rolling_params* p);   /* 0.5: a placeholder, see above */
/* cand_frame and cand_t are host arrays of n_out * 2 entries; dst holds full w x h frames.  VS_MEM_DEVICE only enqueues.  The entries
 * reach the device in the denoise's groups (2048 frames); a destination whose rows do not all start on dwords, or a width that is no
 * multiple of 4, takes the one-pixel-per-lane kernel, with the same result. */
int vs_bgr_rolling_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride, int format,
                         int n_out, const int32_t* cand_frame, const vs_transform* cand_t,
                         const vs_rolling_params* params /* NULL = defaults */,
                         void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* REMAP and LENS-DISTORTION CORRECTION: a lens bends the frame from inside in a way that is constant per clip and calibrated once, which no
 * transform per frame removes.  The correction is a remap through a map of fixed-point positions made once; callers with a fisheye or any
 * other calibrated model bring their own map.
 * THE MAP FORMAT.  A map for `ow x oh` output pixels is `int32_t` pairs `(X, Y)`.
 *
 * - Pixel `(u, v)` is at `map[v * map_stride + 2 * u]` and `+ 1`.
 * - `map_stride` is in `int32_t` elements and is `>= 2 * ow`.
 * - `X` and `Y` are source positions with 5 fraction bits: exactly what `vsd::cv_pos` produces (`CvPos`), `VS_WARP_BILINEAR_CV`'s own positions.
 * - Every int32 value is legal.
 *
 * THE SAMPLE RULE of `vs_bgr_remap_batch`.  Interleaved BGR, every `VS_FMT_BGR*`; `w, h, ow, oh` in 1 .. 32767, `VS_ERR_UNSUPPORTED` beyond,
 * as the rolling-shutter pass does.  One map serves all `n` frames; the map lives where the frames live (`mem`).
 *
 * - Taps sit at `(X >> 5, Y >> 5)` and the three neighbours to the right and below. Fractions are `X & 31`, `Y & 31`.
 * - The blend is `VS_WARP_BILINEAR_CV`'s, operation for operation.
 *   - 8-bit containers: integer weights, `(sum + 512) >> 10`.
 *   - 16-bit containers: fp32 weights `a * b / 1024`, `rintf`, saturated to `vs_format_max_value(format)`.
 * - `VS_BORDER_CLAMP`: each tap's column is clamped to `0 .. w - 1` and its row to `0 .. h - 1`, with weights unchanged. This is the
 *   rolling-shutter pass's rule.
 * - `VS_BORDER_CONSTANT`: a tap outside the frame counts as 0, with weights unchanged. This is `VS_WARP_BILINEAR_CV`'s rule under that border.
 * - Tap index sums are taken so that no int32 `X` or `Y` overflows (`X >> 5` is below 2^26).
 *
 * Hence
 *
 * - (a) The map `X = 32 u, Y = 32 v` with `ow == w, oh == h` returns every frame bit for bit. This holds for samples up to the format's maximum.
 * - (b) Under the clamp border, every output sample lies between the minimum and maximum of the frame's samples in its channel.
 * - (c) Every sample is defined for every map.
 * VS_MEM_DEVICE only enqueues.  A destination whose rows do not all start on dwords, or an `ow` that is no multiple of 4, takes the
 * one-pixel-per-lane kernel, with the same result. */
int vs_bgr_remap_batch(const void* src, size_t src_frame_stride, int n, int w, int h, int src_stride, int format,
                       const int32_t* map, int map_stride, int ow, int oh, int border,
                       void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* THE RADIAL MAP: the Brown-Conrady model with a rational radial term, the same eight coefficients in the same order as OpenCV's distCoeffs
 * (k1, k2, p1, p2, k3, k4, k5, k6).  The output camera is the input camera with its focal lengths scaled by `zoom`.  `border` is what the
 * stabilizer's correction remaps with; the map itself does not depend on it.  Defaults: fx = fy = max(w, h), cx = (w - 1) / 2,
 * cy = (h - 1) / 2, all coefficients 0, zoom 1, VS_BORDER_CLAMP: the identity lens.
 * The rule, per output pixel (u, v).  All arithmetic is fp64, every operation rounds once in the order written, and there is no FMA:
 *   x = ((double)u - cx) / (fx * zoom);      y = ((double)v - cy) / (fy * zoom);
 *   r2 = x * x + y * y;
 *   kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
 *   xy2 = 2 * (x * y);
 *   xd = x * kr + (p1 * xy2 + p2 * (r2 + 2 * (x * x)));
 *   yd = y * kr + (p1 * (r2 + 2 * (y * y)) + p2 * xy2);
 *   X = cv_round_sat((fx * xd + cx) * 32);   Y = cv_round_sat((fy * yd + cy) * 32);
 * cv_round_sat: ties to even, NaN -> 0, saturating to the int32 range.  Only + - * / and rint: VS_MEM_HOST (computed on the host, no device
 * needed) and VS_MEM_DEVICE (a small kernel, enqueue only) give the same bits.  A parameter that is not finite, or an fx, fy or zoom that is
 * not > 0, is VS_ERR_ARG before any work; a denominator that reaches 0 at some pixel is legal input (the rule defines the position through
 * cv_round_sat).  With all eight coefficients 0 and zoom 1 the map is (32 u, 32 v).  w, h in 1 .. 32767; map_stride >= 2 * w.
 * The fisheye (equidistant) model needs a transcendental that is not bit-reproducible and is left to the caller's own map. */
typedef struct vs_lens_params { double fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6, zoom; int border; } vs_lens_params;
void vs_lens_params_default(vs_lens_params* p, int w, int h);
int  vs_lens_map(const vs_lens_params* p, int w, int h, int32_t* map, int map_stride, int mem, void* stream);
/* YCbCr FRAMES: decoders, cameras and encoders speak planar or semi-planar YCbCr, mostly 4:2:0; every other entry point of this library takes
 * interleaved BGR.  The two calls below convert on the device, in front of and behind everything else, under an exact integer rule:
 * BT.601 limited range in 8.8 fixed point, chroma replicated towards BGR and box-averaged towards YCbCr -- bit for bit what the harness
 * programs' apps/video_io.hpp does on the host (vsio::ycbcr_to_bgr, vsio::bgr_to_ycbcr, Reader::unpack, Writer::pack).
 * THE RULE (written once for host and device: video_stabilizer_amd/csrc/vs_ycbcr.hpp).  bits = vs_format_bits(format), sh = bits - 8,
 * maxv = vs_format_max_value(format); every `>> 8` is an arithmetic shift, a floor.
 *
 * To BGR, pixel (x, y):
 * - c = Y[y][x] - (16 << sh), d = Cb - (128 << sh), e = Cr - (128 << sh).
 * - Cb and Cr are read at (x >> sub_x, y >> sub_y).  Without chroma planes both are 128 << sh.
 * - r = clamp((298 c + 409 e + 128) >> 8, 0, maxv)
 * - g = clamp((298 c - 100 d - 208 e + 128) >> 8, 0, maxv)
 * - b = clamp((298 c + 516 d + 128) >> 8, 0, maxv)
 * - Every container value is legal input; all sums stay inside int32 at 16 bits.
 *
 * To YCbCr:
 * - Every BGR sample is first cut to min(sample, maxv).
 * - y  = clamp(((66 r + 129 g + 25 b + 128) >> 8) + (16 << sh), 0, maxv)
 * - cb = clamp(((-38 r - 74 g + 112 b + 128) >> 8) + (128 << sh), 0, maxv)
 * - cr = clamp(((112 r - 94 g - 18 b + 128) >> 8) + (128 << sh), 0, maxv)
 * - Chroma cell (cx, cy) averages the bx x by per-pixel values, bx = 1 << sub_x, by = 1 << sub_y, of the pixels
 *   (min(cx bx + dx, w - 1), min(cy by + dy, h - 1)): (sum + cnt / 2) / cnt with cnt = bx by.
 * - Chroma planes are (w + sub_x) >> sub_x by (h + sub_y) >> sub_y.
 *
 * Hence
 *
 * - (a) Gray BGR (b == g == r) gives neutral chroma, 128 << sh, exactly.
 * - (b) With no chroma planes, to-BGR gives b == g == r.
 * - (c) Every output is defined for every input.
 * - (d) Both directions equal apps/video_io.hpp on every input.
 *
 * THE DESCRIPTOR.  I420, YV12, NV12, NV21, I422, I444 and luma-only frames are all instances of one struct; there is no enum of layouts.
 * Elements are uint8_t at 8 bits and uint16_t above, with the samples in the LOW bits (y4m's layout, and VS_FMT_BGR10 / 12's).  P010's
 * high-bit alignment is out of scope, as are BT.709 and full-range matrices and sited chroma filters: each is a rule of its own.
 * With c_step == 2 the two chroma pointers are one element apart and a row of the pair is one run of 2 * chroma-width elements. */
typedef struct vs_ycbcr_planes {
    void *y, *cb, *cr;          /* frame 0's first samples; cb == cr == NULL: luma only (y4m "mono") */
    int y_stride, c_stride;     /* elements between rows */
    int c_step;                 /* elements between chroma samples of a row: 1 planar, 2 interleaved (NV12: cr == cb + 1, NV21: cb == cr + 1) */
    int sub_x, sub_y;           /* log2 subsampling, 0 or 1 each: (1,1) 4:2:0, (1,0) 4:2:2, (0,0) 4:4:4 */
    size_t y_frame_stride, c_frame_stride;   /* elements between frames */
} vs_ycbcr_planes;
/* n frames of w x h, w, h in 1 .. 32767 (VS_ERR_UNSUPPORTED beyond, as the remap); format: a VS_FMT_BGR* (VS_FMT_GRAY8: VS_ERR_ARG).
 * VS_ERR_ARG also for a c_step that is not 1 or 2 (or 2 with chroma pointers that are not neighbours), a sub_* that is not 0 or 1, exactly
 * one of cb / cr being NULL, and strides shorter than a row (frame strides shorter than a frame, for n > 1).  VS_MEM_DEVICE only enqueues;
 * VS_MEM_HOST stages every plane's span as one dense copy (an interleaved pair is one span) and synchronises.  Destination bytes outside
 * the rows' own samples are never written; with NULL chroma no chroma is written.  Where w is a multiple of 4 and every row of every
 * plane and of the BGR side starts on a dword, a lane takes four columns with dword accesses; anything else takes one chroma cell per
 * lane, element by element, with the same result. */
int vs_ycbcr_to_bgr_batch(const vs_ycbcr_planes* src, int n, int w, int h, int format,
                          void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
int vs_bgr_to_ycbcr_batch(const void* src, size_t src_frame_stride, int n, int w, int h, int src_stride, int format,
                          const vs_ycbcr_planes* dst, int mem, void* stream);
/* RESIZE: frames from one size to another, a pass of its own behind everything (the delivery size of a transcode).
 *
 * THE RESIZE RULE.  This build's specification; it is not OpenCV's `cv::resize` binary (its 8-bit linear path rounds twice, its 16-bit path
 * is float).
 *
 * - It applies to interleaved BGR, every `VS_FMT_BGR*`.
 * - Source is `sw x sh`, destination `dw x dh`, each 1 .. 32767.
 * - It is separable. Each axis gets a TAP TABLE from integers only, so host and device agree by construction.
 * - A table entry is a first index `i0[d]`, a count `n[d] >= 1` and weights `wt[d][k] >= 0` with `sum_k wt[d][k] == 4096` exactly.
 * - The filter is chosen per call: `VS_RESIZE_LINEAR` or `VS_RESIZE_AREA`.
 *
 * LINEAR, any ratio.
 *
 * - With 64-bit integers, `num = (2 d + 1) s - dn` and `p = floor(num * 4096 / (2 dn))`, floor towards minus infinity.
 * - `p` is clamped to `[0, (s - 1) * 4096]`. `i = p >> 12`, `f = p & 4095`.
 * - The taps are `(i, 4096 - f)` and `(min(i + 1, s - 1), f)`. The table lists the second tap only where `f != 0`.
 * - Here `s` is the source extent and `dn` the destination extent of that axis.
 *
 * AREA, only where `dn <= s <= 8 dn` on that axis; otherwise `VS_ERR_UNSUPPORTED`.
 *
 * - In units of `1 / dn` source pixels, destination cell `d` covers `[d s, (d + 1) s)`.
 * - Its taps are the source pixels `k = floor(d s / dn) .. floor(((d + 1) s - 1) / dn)`.
 * - `cum_k = min((k + 1) dn, (d + 1) s) - d s`.
 * - `C_k = floor((cum_k * 4096 + floor(s / 2)) / s)`.
 * - `wt_k = C_k - C_(k-1)`, with `C = 0` before the first tap.
 * - Hence the weights sum to 4096 and `n <= floor(s / dn) + 2 <= 10`.
 *
 * SAMPLE.
 *
 * - `v' = min(v, max_value)`.
 * - Per channel, `H(y, d) = sum_k wx[d][k] * v'(y, ix0[d] + k)`. This is exact and below 2^28.
 * - `V = sum_j wy[e][j] * H(iy0[e] + j, d)`. This is exact. It fits unsigned 32 bits for 8-bit frames including the rounding term:
 *   `4096 * 4096 * 255 + 2^23 < 2^32`. Deeper frames take 64 bits.
 * - `out = (V + 2^23) >> 24`. There is one rounding per sample and it happens here.
 *
 * Hence
 *
 * - (a) `dw == sw && dh == sh` is the identity, bit for bit, under both filters (for samples up to the format's maximum).
 * - (b) A constant frame stays constant.
 * - (c) Every output lies within the min .. max of its taps, so no sample exceeds `max_value`.
 * - (d) AREA at an integer factor `k` gives equal weights when `4096 % k == 0`. Factor 2 gives `(a + b + c + d + 2) >> 2`.
 * - (e) LINEAR at `sw == 2 dw` equals AREA there.
 * - (f) LINEAR 4 -> 8 has weights `4096 | 3072,1024 | 1024,3072 | ... | 4096`.
 * - (g) AREA 7 -> 3 has the tables `(0: 1755,1756,585) (2: 1170,1756,1170) (4: 585,1756,1755)`. */
#define VS_RESIZE_LINEAR 0
#define VS_RESIZE_AREA 1
/* One axis' table as the kernels use it, on the host (no device needed): `i0[d]`, `n[d]` and `wt[d * 10 + k]`, `k < n[d]`, for
 * every destination index of the axis `s -> d`; weights past `n[d]` are written as 0.  `VS_ERR_ARG` for NULL arrays, an extent outside 1 .. 32767 or an unknown
 * filter; `VS_ERR_UNSUPPORTED` for AREA outside `d <= s <= 8 d`. */
int vs_resize_taps(int s, int d, int filter, int32_t* i0, int32_t* n, uint16_t* wt /* d x 10 */);
/* n frames of sw x sh -> n frames of dw x dh.  Argument checks, staging and VS_MEM_* as vs_bgr_gain_batch and vs_bgr_remap_batch.
 * n == 0 is VS_OK without a launch.  src == dst is VS_ERR_ARG (out of place; overlapping ranges are the caller's to avoid).  An extent
 * above 32767, or AREA outside its range (the message names the axis), is VS_ERR_UNSUPPORTED before any work.  Both axes' tables are built
 * once per call on the device and shared by the call's frames.  VS_MEM_DEVICE only enqueues. */
int vs_bgr_resize_batch(const void* src, size_t src_frame_stride, int n, int sw, int sh, int src_stride, int format, int filter,
                        void* dst, size_t dst_frame_stride, int dw, int dh, int dst_stride, int mem, void* stream);
/* DEFLICKER: a frame's exposure is pulled to the average exposure of a window of frames, the exposure ratio of two frames being measured
 * at the same scene points through their measured motions (a pan changes a whole-frame sum because the content changes).  Interleaved
 * BGR, every VS_FMT_BGR*, frames up to 32767 a side (VS_ERR_UNSUPPORTED beyond, as in the fill); s = bits - 8.  The rule:
 *   - Candidates: output frame o has n_cand (1 .. 16) candidates (cand_frame, cand_t), exactly as in vs_bgr_denoise_batch.  Candidate 0
 *     is the target frame k itself and its transform is ignored; a negative index ends the list; cand_t is in VS_WARP_BILINEAR_CV's
 *     forward convention.
 *   - Lattice: step is 1 .. 64 (default 4); lattice pixels are those with x % step == 0 && y % step == 0;
 *     L = ceil(w / step) * ceil(h / step).
 *   - Pair statistics of candidate j >= 1: with M = vs_cv_inverse_matrix(cand_t) lattice pixel (x, y) lies in candidate j at
 *     qx = rint((M0 x + M1 y) + M2), qy = rint((M3 x + M4 y) + M5) (doubles, that order, no fma, ties to even: the deblur's
 *     nearest-sample position).  The pair counts iff qx, qy are finite, 0 <= qx <= w-1, 0 <= qy <= h-1 and every one of the six samples
 *     v (three of p = the target at (x, y), three of q = the candidate at (qx, qy)) has 0 < (v >> s) < 255: neither black nor clipped
 *     at 8-bit precision, which also rejects samples above the format's maximum.  Per candidate seven uint64_t: count, a_c = sum p_c,
 *     b_c = sum q_c (count < 2^30, sums < 2^46; integer sums, so the order of the reduction cannot matter).  A NaN or infinite map
 *     counts nothing.
 *   - Gains of output frame o, unsigned 64-bit with floor division: candidate j is USED iff count_j >= max(1, L / 16) (then every
 *     a_j,c >= count_j > 0);  r_j,c = clamp((2 * 32768 * b_j,c + a_j,c) / (2 * a_j,c), 16384, 65536)  (every term below 2^63);  with m
 *     used candidates  G_c = (2 * (32768 + sum_j r_j,c) + (1 + m)) / (2 * (1 + m)):  the rounded mean of the window's exposures
 *     relative to k, with k itself included as 32768.  (Caller-made statistics with a_j,c == 0 under a used count, which the
 *     statistics call cannot produce, give r_j,c = 32768.)
 *   - Applied sample: min((v * G_c + 16384) >> 15, max_value) in unsigned 32-bit (65535 * 65536 + 16384 < 2^32).  A frame whose three
 *     gains are all 32768 is left as it is, bit for bit, including samples above the maximum.
 *   - Hence (a) n_cand == 1, a list that ends at once, candidates that lie outside the frame and candidates with fewer than
 *     max(1, L / 16) counted pairs give the frame back bit for bit; (b) identical frames under identity maps come back bit for bit;
 *     (c) constant frames of 100 (target) and 200 (one candidate) give r = 65536, G = 49152 and every sample 150;
 *     (d) 16384 <= G_c <= 65536 whatever the content and the maps; (e) a candidate that is frame k under an integer shift with every
 *     sample halved exactly gives r_j = 16384.
 * A step outside 1 .. 64 is VS_ERR_ARG, before any device work. */
typedef struct vs_deflicker_params { int step; } vs_deflicker_params;
void vs_deflicker_params_default(vs_deflicker_params* p);   /* 4 */
/* stats[(o*n_cand + j)*8 + {0: count, 1..3: a_B,a_G,a_R, 4..6: b_B,b_G,b_R, 7: 0}]; entry j = 0 is all zero; `stats` lives in `mem`;
 * cand_frame and cand_t are host arrays of n_out * n_cand entries.  VS_MEM_DEVICE only enqueues. */
int vs_bgr_exposure_stats_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride, int format,
                                int n_out, int n_cand, const int32_t* cand_frame, const vs_transform* cand_t,
                                const vs_deflicker_params* params /* NULL = defaults */, uint64_t* stats, int mem, void* stream);
/* gains[4*o + {0..2: G_B,G_G,G_R, 3: m}]; stats and gains live in `mem`.  Statistics in host memory beyond the rule's bounds
 * (count >= 2^30, a sum >= 2^46) are VS_ERR_ARG; in device memory the arithmetic wraps modulo 2^64 and G_c keeps its range. */
int vs_exposure_gains_batch(const uint64_t* stats, int n_out, int n_cand, int w, int h,
                            const vs_deflicker_params* params /* NULL = defaults */, uint32_t* gains, int mem, void* stream);
/* frame i scaled by gains[4*i ..] (gains[4*i + 3] is not read); dst may be src (in place: every sample is read and written by the same
 * thread); w x h is the window the caller hands over, any size.  A gain outside 16384 .. 65536 in host memory is VS_ERR_ARG, before
 * any device work; gains in device memory are never seen by the host: the kernel clamps them to that range. */
int vs_bgr_gain_batch(const void* src, size_t src_frame_stride, int n, int w, int h, int src_stride, int format,
                      const uint32_t* gains, void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* SCENE-CUT DETECTION: the frame difference of two consecutive frames taken through their measured motion.  The aligner is no cut detector:
 * across a hard cut it often converges to some small similarity and reports success.  Inside a scene the difference through the measured
 * motion is close to zero however hard the camera shakes; across a cut it is large whatever the aligner made of it.
 *
 * THE SCENE-CUT RULE (also vs_scene.hip).
 * Interleaved BGR, every VS_FMT_BGR*, frames up to 32767 a side; s = bits - 8.
 *   - PARAMETERS.  step is 1 .. 64 (default 4, the deflicker's lattice); threshold is 1 .. 255, in 8-bit levels (default 32: above a 20 % exposure
 *     jump and below every cut of the synthetic clips it was measured on -- a starting value, not a calibrated one).
 *   - PAIR AND LATTICE.  A pair is (target frame, candidate frame, forward transform t in VS_WARP_BILINEAR_CV's convention): what a deflicker or
 *     denoise candidate list gives for candidate 1.  The lattice pixels are those with x % step == 0 && y % step == 0;
 *     L = ceil(w / step) * ceil(h / step).
 *   - POSITION.  With M = vs_cv_inverse_matrix(t) lattice pixel (x, y) lies in the candidate at qx = rint((M0 x + M1 y) + M2),
 *     qy = rint((M3 x + M4 y) + M5): doubles, that order, no fma, ties to even -- the deflicker's and deblur's nearest-sample position.  The
 *     lattice pixel COUNTS iff qx, qy are finite, 0 <= qx <= w - 1 and 0 <= qy <= h - 1.  There is no level test: black and clipped samples count.
 *   - STATISTIC.  With v' = min(v, max_value) >> s, each pair yields two uint64: count, and sad = the sum over the counted lattice pixels of
 *     sum_c |p'_c - q'_c| (p the target at (x, y), q the candidate at (qx, qy)).  count < 2^30 and sad < 3 * 255 * 2^30; integer sums: the
 *     order of the reduction cannot matter.  A NaN or infinite map counts nothing.
 *   - DECISION.  Unsigned 64-bit: the pair is a CUT iff count < max(1, L / 16) or sad > 3 * threshold * count.  The inequality is strict:
 *     equality is no cut.  Too little overlap is a cut: nothing shows that the frames are one scene, and nothing could be borrowed from the
 *     candidate anyway.
 *   - HENCE (a) identical frames under the identity give sad == 0; (b) a frame and its copy shifted by whole pixels, under that shift, give
 *     sad == 0 and count = the overlap's lattice count; (c) constant frames of 100 and 130 give sad == 90 * count.
 * The default threshold, 32, comes from SYNTHETIC clips (within a scene at most 1.8 levels, a 20 % exposure jump 25,
 * cuts 48 and more) and is a starting value: footage with flashes or hard exposure steps may want it higher, low-contrast footage lower.
 * A step outside 1 .. 64 or a threshold outside 1 .. 255 is VS_ERR_ARG, before any device work. */
typedef struct vs_scene_params { int step; int threshold; } vs_scene_params;
void vs_scene_params_default(vs_scene_params* p);   /* {4, 32}: a starting value, see above */
/* stats[2*i + {0: count, 1: sad}] of pair i = (frame pair_frames[2*i] of the batch as the target, frame pair_frames[2*i + 1] as the
 * candidate, pair_t[i]); `stats` lives in `mem`; pair_frames and pair_t are host arrays.  A pair may name a frame twice and pairs may come
 * in any order.  n_pairs == 0 is VS_OK and launches nothing; a frame index outside 0 .. n_src-1 is VS_ERR_ARG.  VS_MEM_DEVICE only
 * enqueues. */
int vs_bgr_scene_stats_batch(const void* src, size_t src_frame_stride, int n_src, int w, int h, int src_stride, int format,
                             int n_pairs, const int32_t* pair_frames /* 2 per pair: target, candidate */, const vs_transform* pair_t,
                             const vs_scene_params* params /* NULL = defaults */, uint64_t* stats /* 2 per pair */, int mem, void* stream);
/* The rule's decision, on the host (no device needed): cut[i] = 1 iff pair i is a cut.  stats and cut are host arrays. */
int vs_scene_cuts(const uint64_t* stats, int n_pairs, int w, int h, const vs_scene_params* params /* NULL = defaults */, uint8_t* cut);
/* FIDELITY STATISTICS of image pairs: the squared error per channel and on gray, and an integer SSIM over 8 x 8 windows.  What the stabilization
 * literature scores a clip by -- ITF, the mean PSNR between consecutive output frames -- and what denoise and deblur work reports against a
 * reference clip, PSNR and SSIM, are all integer sums over two frames that already lie in device memory: one pass that reads each image once.
 *
 * THE FIDELITY RULE (also vs_fidelity.hip).
 *   - SCOPE.  Interleaved BGR, every VS_FMT_BGR*, images of 1 .. 32767 pixels a side; s = bits - 8.  Every sample is first v' = min(v, max_value).
 *   - PAIR.  A pair is (image a, image b), both w x h.  Each side has its own row stride and frame stride.  An image may be a window of a larger
 *     frame: pass its origin pointer with the frame's strides.  Row starts may therefore fall on any byte (8-bit) or any element (16-bit).
 *   - GRAY.  g = min(((B' * 3735 + G' * 19235 + R' * 9798 + 16384) >> 15) >> s, 255), in unsigned 32-bit arithmetic: vs_bgr_to_gray's weights.  The
 *     largest value is 65535 * 32768 + 16384 < 2^32.
 *   - WORDS.  Each pair gives six uint64: words 0 .. 2 sse_b, sse_g, sse_r = the sum over all pixels of (a'_c - b'_c)^2, at the format's own
 *     precision; word 3 sse_y = the same sum on g; word 4 n_win; word 5 ssim_sum, an int64 in two's complement.
 *   - WINDOWS.  8 x 8 at a stride of 4: nwx = w >= 8 ? (w - 8) / 4 + 1 : 0, nwy likewise from h, n_win = nwx * nwy.  Window (i, j) covers x in
 *     4i .. 4i + 7 and y in 4j .. 4j + 7.  Pixels right of, or below, the last window belong to no window; they still count in the four SSE words.
 *   - PER WINDOW.  All on g, all in int32.  s1 = sum g_a, s2 = sum g_b, ss = sum (g_a^2 + g_b^2), s12 = sum g_a g_b;
 *       vars = 64 ss - s1^2 - s2^2,  cov = 64 s12 - s1 s2;  c1 = 26634, c2 = 239708 ((0.01 * 255)^2 * 64^2 and (0.03 * 255)^2 * 64^2, rounded);
 *       A = 2 s1 s2 + c1,  B = 2 cov + c2,  C = s1^2 + s2^2 + c1,  D = vars + c2;
 *       q = rint(((double)(int64)(A * B) / (double)(int64)(C * D)) * 65536.0): the conversions and the division correctly rounded, no fma, ties to
 *       even.  ssim_sum = sum q.
 *   - BOUNDS.  s1, s2 <= 16320 and ss <= 8 323 200; each of vars, |cov|, A, |B|, C, D is at most 532 924 508 < 2^31 and the products stay below
 *     2^59; C >= c1 and D >= c2, so both are positive; |q| <= 65536, because 2 s1 s2 <= s1^2 + s2^2 and 2 |cov| <= vars.
 *     sse_c <= 65535^2 * 2^30 < 2^62, n_win < 2^26, |ssim_sum| < 2^42.
 *   - HENCE (a) a == b gives zero SSE words and ssim_sum = 65536 * n_win; (b) 8-bit constant images of 100 and 130 give 900 w h in each SSE word and
 *     q = 63344 in every window; (c) all-0 against all-maximum gives max_value^2 * w h per channel, 65025 w h for sse_y and q = 7; (d) an 8-bit
 *     checkerboard of 0 / 255 against its inverse gives q = -65300; (e) exchanging a and b changes no word.
 *   - Integer sums only: the order of the reduction cannot matter, so results are identical from run to run.
 * THE SCORES (vs_fidelity_scores, on the host).  With peak = max_value and N = (double)w * (double)h:
 *     psnr_c = 10.0 * log10((peak * peak * N) / (double)sse_c);  psnr pools the three channels: 3 N and sse_b + sse_g + sse_r;  psnr_y uses a peak
 *     of 255 and sse_y;  a zero SSE gives HUGE_VAL;  ssim = (double)ssim_sum / (65536.0 * n_win), and NaN when n_win == 0.
 * The constants come from the usual SSIM derivation with population variances over 64 samples; they are this build's specification.  Values are
 * close to, but not equal to, what other tools print: those scale c1 differently, weight the window with a Gaussian and finish in fp32. */
typedef struct vs_fidelity_score { double psnr_b, psnr_g, psnr_r, psnr, psnr_y, ssim; } vs_fidelity_score;
/* stats[6*i ..] of pair i = (image pair_frames[2*i] of the batch at `a`, image pair_frames[2*i + 1] of the batch at `b`).  Both batches hold w x h
 * images in `format`, n_a / n_b of them, frame strides and row strides in elements; `b` may be the batch at `a` (a host batch is then staged
 * once).  `stats` lives in `mem`; pair_frames is a host array.  Pairs may repeat, may come in any order and may name one image twice.
 * n_pairs == 0 is VS_OK and launches nothing.  An index outside its batch, a stride below 3 w, VS_FMT_GRAY8 or a size outside 1 .. 32767 is
 * VS_ERR_ARG, before any device work.  VS_MEM_DEVICE only enqueues. */
int vs_bgr_fidelity_batch(const void* a, size_t a_frame_stride, int n_a, int a_stride,
                          const void* b, size_t b_frame_stride, int n_b, int b_stride,
                          int w, int h, int format, int n_pairs, const int32_t* pair_frames /* 2 per pair: into a, into b */,
                          uint64_t* stats /* 6 per pair, in mem */, int mem, void* stream);
/* The rule's scores, on the host (no device needed): stats and scores are host arrays. */
int vs_fidelity_scores(const uint64_t* stats, int n_pairs, int w, int h, int format, vs_fidelity_score* scores);
/* PHASE-COMPENSATED SHARPENING behind VS_WARP_BILINEAR_CV.  A bilinear resample is a two-tap box filter per axis, [1 - f, f], whose blur
 * depends on the sub-pixel phase f: none at f = 0, most at f = 1/2.  In stabilised video every pixel's phase drifts from frame to frame, so
 * the output's sharpness pulses.  The warp's positions carry five fraction bits, a = X & 31, b = Y & 31; the filter [1 - a/32, a/32] has
 * variance a (32 - a) / 1024 pixel^2, and its second-order inverse is identity - (variance / 2) [1, -2, 1]: a five-point stencil whose two
 * weights are known per pixel from the warp's own matrix.
 *
 * THE SHARPEN RULE (also vs_sharpen.hip).
 *   - SCOPE.  Interleaved BGR, every VS_FMT_BGR*, frames up to 32767 a side (VS_ERR_UNSUPPORTED beyond, as the fill).
 *   - IMAGE AND WINDOW.  The input is an image of roi_w x roi_h pixels: the window [roi_x, roi_x + roi_w) x [roi_y, roi_y + roi_h) of a
 *     w x h output frame that VS_WARP_BILINEAR_CV made under the forward transform t.  (x, y) below are full-frame coordinates, as in the
 *     fill.
 *   - POSITIONS.  X, Y (int32, five fraction bits) and sx = X >> 5, sy = Y >> 5 are the fill's, to the letter (see
 *     vs_bgr_image_warp_fill_batch): M = vs_cv_inverse_matrix(t); cvRound saturates to int32, NaN gives 0, and + 16 and X0 + adelta wrap.
 *     a = X & 31, b = Y & 31, va = a (32 - a), vb = b (32 - b): both lie in 0 .. 256.
 *   - COVERED.  A pixel is covered iff all four taps lie in the frame (the fill's candidate-0 rule): 0 <= sx, sx + 1 <= w - 1, 0 <= sy,
 *     sy + 1 <= h - 1.
 *   - ELIGIBLE.  A pixel is eligible iff it is not on the window's outermost row or column, it is covered, and its four edge neighbours
 *     (x +- 1, y) and (x, y +- 1) are covered.
 *   - DELTA.  For an eligible pixel and each channel, with raw samples c, l, r, u, d (no clamp of the taps):
 *     num = strength * (va * (2c - l - r) + vb * (2c - u - d)), delta = (num + 16384) >> 15, an arithmetic shift.
 *   - OUTPUT.  out = c if the pixel is not eligible or delta == 0; otherwise out = clamp(c + delta, 0, max_value).
 *   - STRENGTH.  1 .. 32 in sixteenths, default 16: the filter's own variance, the derivation above, not a tuned value.  Anything else
 *     is VS_ERR_ARG.
 *   - BOUND.  |num| <= 32 * 512 * 131070 = 2 147 450 880 < 2^31 - 16384: int32 is enough throughout.
 *   - HENCE (a) under the identity or any whole-pixel shift every pixel comes back bit for bit; (b) a constant image, and an image linear
 *     in x and y, come back bit for bit under any map; (c) pixels the frame's own source does not cover (border, fill, inpaint), and their
 *     edge neighbours, come back bit for bit; (d) a sample above max_value is changed only where delta != 0; (e) a NaN map gives
 *     X = Y = 16 >> 5 = 0 everywhere: every pixel is covered and va = vb = 0, so the image comes back bit for bit. */
typedef struct vs_sharpen_params { int strength; } vs_sharpen_params;
void vs_sharpen_params_default(vs_sharpen_params* p);   /* 16 */
/* n images of roi_w x roi_h at src (rows of src_stride elements, src_frame_stride elements apart), image i under t[i], to dst in the same
 * shape (dst_stride, dst_frame_stride).  n == 0 is VS_OK without a launch.  The stencil cannot run in place: a src range that overlaps the
 * dst range is VS_ERR_ARG.  A window outside the w x h frame is VS_ERR_ARG.  t is a host array.  VS_MEM_DEVICE only enqueues. */
int vs_bgr_sharpen_batch(const void* src, size_t src_frame_stride, int n, int w, int h, int format,
                         const vs_transform* t /* host, n */, const vs_sharpen_params* params /* NULL = defaults */,
                         int roi_x, int roi_y, int roi_w, int roi_h, int src_stride,
                         void* dst, size_t dst_frame_stride, int dst_stride, int mem, void* stream);
/* ---- Inpaint of what the border fill leaves open: a coverage index and an exact-integer push-pull over the output window ----
 * THE RULE.  VS_WARP_BILINEAR_CV conventions, 3 channels, 8- and 16-bit containers, every VS_FMT_BGR*, windows up to 32767 a side.
 *   - COVERAGE INDEX.  Output frame o has n_cand (1 .. 16) candidates exactly as in vs_bgr_image_warp_fill_batch: each a forward
 *     transform, a negative frame index ends the list, candidate 0 is the frame itself.  Only the sign of an index is looked at.  For
 *     window pixel (x, y), cov = 1 + c, where c is the first candidate that COVERS the pixel by the fill's int32 rule, unchanged: the
 *     positions X, Y of cv::warpAffine's tables, saturating cvRound with NaN -> 0, wrapping additions, all four taps inside w x h,
 *     full-frame coordinates under the ROI.  cov = 0 if no candidate covers the pixel.
 *   - INPAINT of one W x H window in place, given a byte mask m0 (non-zero = keep).  Pixel values outside the mask are never read.
 *       Levels: W_0 = W, H_0 = H, W_{l+1} = (W_l + 1) >> 1, H_{l+1} = (H_l + 1) >> 1, up to the level L with W_L = H_L = 1.
 *       Push, l -> l+1, per channel: the children of (X, Y) are the pixels (2X+i, 2Y+j), i, j in {0, 1}, that exist at level l and
 *         have m_l != 0; n is their number and s their sum.  n == 0: m_{l+1} = 0 and the value is unused.  Otherwise m_{l+1} = 1 and
 *         the value is (2 s + n) / (2 n), floor division: the rounded mean (unsigned 32-bit is enough; the result fits the container).
 *       If m_L == 0 (no kept pixel in the window) the window is left untouched.
 *       Pull, l = L-1 .. 0 (level l+1 is completely defined by then): a pixel (x, y) with m_l == 0 becomes
 *         (9 P(px,py) + 3 P(qx,py) + 3 P(px,qy) + P(qx,qy) + 8) >> 4 over level l+1, where px = x >> 1,
 *         qx = clamp(px + (x & 1 ? 1 : -1), 0, W_{l+1} - 1), and py, qy are formed the same way from y and H_{l+1}.
 *   - Hence (a) kept pixels come back bit for bit; (b) every inpainted sample lies between the minimum and the maximum of the kept
 *     samples of its channel, so max_value never comes into it; (c) if the kept pixels have one colour the whole window gets it; (d) an
 *     all-kept window and an all-open window come back bit for bit; (e) the result does not depend on the prior content of open pixels.
 * cov: n_out indices of roi_h rows of cov_stride bytes, cov_frame_stride bytes apart, in `mem`; cand_frame and cand_t are host arrays of
 * n_out * n_cand entries.  VS_MEM_DEVICE only enqueues. */
int vs_bgr_fill_coverage_batch(int w, int h, int n_out, int n_cand, const int32_t* cand_frame, const vs_transform* cand_t,
                               int roi_x, int roi_y, int roi_w, int roi_h, uint8_t* cov, size_t cov_frame_stride, int cov_stride,
                               int mem, void* stream);
/* n windows of w x h pixels in place (frame_stride, stride in elements; mask_frame_stride, mask_stride in bytes); img and mask live in
 * `mem`.  The call takes its scratch from the device and returns when the work is done. */
int vs_bgr_inpaint_batch(void* img, size_t frame_stride, int n, int w, int h, int stride, int format, const uint8_t* mask,
                         size_t mask_frame_stride, int mask_stride, int mem, void* stream);
/* same sampling, float output (typed like image_warp); dst interleaved f32 */
int vs_bgr_image_warp_f32(const void* src, int w, int h, int src_stride, int channels, int bits,
                          const vs_transform* t, int mode, int border,
                          float* dst, int dst_stride, int mem, void* stream);
/* cv::cvtColor(BGR2GRAY) stand-in (alignment.cpp:212): (B*3735+G*19235+R*9798+16384)>>15, then >>shift_to_8 */
int vs_bgr_to_gray(const void* src, int w, int h, int src_stride, int bits, int shift_to_8,
                   uint8_t* dst, int dst_stride, int mem, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense optical flow and the flow-based jitter score (eval_jitter.cpp:43-70, grid_search_align.cpp:27-60)
 * ------------------------------------------------------------------------------------------
 * Two-frame polynomial-expansion flow (Farneback 2003) with cv::calcOpticalFlowFarneback's parameter meanings.  OpenCV is not
 * part of this build: the arithmetic (layer sizes, pyramid blur, border rule, regularisation of the 2x2 solve) is this build's
 * own specification, stated in the header comment of vs_flow.hip and restated in numpy by tests/_flow_ref.py, which the kernels
 * equal bit for bit.  Scores are this build's Farneback, not OpenCV's binary.
 * Fields as OpenCV names them; levels counts the layers ABOVE the frame (levels + 1 layers in all).  flags: 0 only (box window,
 * no initial flow); anything else is VS_ERR_UNSUPPORTED.  Limits: winsize 1..31, poly_n 1..7, levels 0..15.  The pyramid blur of a
 * layer has at most 257 taps (pyr_scale ^ k >= 1/86): parameters in range that ask for more make a handle, and vs_flow_compute /
 * vs_flow_jitter return VS_ERR_UNSUPPORTED before they touch the device or their outputs. */
typedef struct vs_flow_params {
    double pyr_scale;
    int    levels;
    int    winsize;
    int    iterations;
    int    poly_n;
    double poly_sigma;
    int    flags;
} vs_flow_params;
/* the reference's call: 0.5, 3, 15, 3, 5, 1.2, 0 */
void vs_flow_params_default(vs_flow_params* p);
/* A handle owns one HIP stream and its device scratch (grown on demand, at most about 2 GiB per chunk of frames: clips are
 * processed in chunks sharing one frame).  Single-threaded like the other handles.  NULL on failure (vs_last_error).
 * The handle's stream is not ordered against the caller's: VS_MEM_DEVICE inputs must be complete before a call (see
 * vs_aligner_wait_stream); every call returns after its device work has finished. */
typedef struct vs_flow vs_flow;
vs_flow* vs_flow_create(const vs_flow_params* params /* NULL = defaults */, int device);
void     vs_flow_destroy(vs_flow* f);
/* Dense flow from prev to next (u8 gray, w x h, row stride `stride`): flow[y*flow_stride + 2x + {0,1}] = (dx, dy) with
 * prev(x, y) ~ next(x + dx, y + dy); flow_stride in floats (>= 2w).  Both images and the flow live in `mem`.  Synchronises. */
int vs_flow_compute(vs_flow* f, const uint8_t* prev, const uint8_t* next, int w, int h, int stride, int mem, float* flow,
                    int flow_stride);
/* The reference's jitter statistic of n >= 2 frames (frame i at frames + i*frame_stride ELEMENTS; any VS_FMT_*, BGR reduced to
 * gray by vs_bgr_to_gray's rule shifted to 8 bits): pair_medians[i] (host, n-1 values) = element (w*h)/2 of the magnitudes of
 * the flow from frame i to frame i+1, selected exactly on the device; *median = their median (mean of the two middle values
 * for an even count).  Synchronises. */
int vs_flow_jitter(vs_flow* f, const void* frames, size_t frame_stride, int n, int w, int h, int stride, int format, int mem,
                   float* pair_medians, double* median);

/* Test hook, not part of the reference's surface: fault injection for the library's own device / pinned-host allocations.
 * vs_test_fail_alloc(k), k > 0: the k-th allocation the library makes from now on (any handle, any thread) fails once with
 * out-of-memory, and the call it belongs to returns VS_ERR_HIP; k < 0: the |k|-th allocation THROWS std::bad_alloc instead -- a host
 * allocation failing at that point of the call, which must come back as VS_ERR_NOMEM (no exception crosses this boundary); k = 0
 * disarms.  Returns the number of allocations made since the
 * previous call of this function.  The environment variable VS_TEST_FAIL_ALLOC=k (honoured only together with VS_TEST_HOOKS=1) arms it at load time for programs that cannot
 * call it.  tests/test_alloc_failure_gpu.py walks k over every allocation of the engine-level calls. */
/* VS_TEST_POISON_ALLOC=<byte> in the environment (read once; honoured only together with VS_TEST_HOOKS=1): every fresh device allocation starts filled with that byte, so that a result
 * which depends on memory the library never wrote changes with the byte (tests/test_uninitialised_memory_gpu.py). */
int vs_test_fail_alloc(int k);

/* Debug build only (tools/build_variant.sh bounds: -DVS_DEBUG_BOUNDS; the reference's "bounds asserts in debug kernels").
 * In that build the LDS / scratch arrays of the selection, gather, exchange, warp-tile and FFT-line code are indexed through a
 * checked accessor: an out-of-range index is recorded (first one per source file: site id, index, limit, workgroup, thread) and
 * the access is redirected to element 0 -- reported, never executed, nothing traps.  vs_debug_bounds_check() synchronises the
 * device, returns the number of violations since the previous call (0 = clean) with the first one described in vs_last_error(),
 * and clears the record.  vs_debug_bounds_selftest() commits one violation on purpose (site 900, index 11 of 8) and returns 202.
 * In the regular library both return VS_ERR_UNSUPPORTED, and the kernels carry no checks (identical instruction streams). */
int vs_debug_bounds_check(void);
int vs_debug_bounds_selftest(void);

/* Profiling aid, not part of the reference's surface: device-to-device copy of floor(bytes/12)*12 bytes
 * with 12-byte accesses per lane, used to calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE for the warp
 * kernel's access width (tools/calibrate_counters.py). */
int vs_calib_copy12(const void* src_dev, void* dst_dev, size_t bytes, void* stream);
/* Profiling aid: the shader clock as a kernel sees it.  Launches one VALU-bound probe kernel (2048 workgroups of dependent fmas,
 * ~0.3 ms) on `stream` of the current device and returns delta s_memtime / delta s_memrealtime x 100 MHz of its first wave in
 * *shader_mhz (MI355X_MICROARCH.md: the pair of counters that shows DVFS give-back); synchronises the stream.  bench.py issues it
 * directly behind its timed loop, so the figure is the clock the timed kernels ran at. */
int vs_shader_clock_probe(void* stream, double* shader_mhz);

/* ------------------------------------------------------------------------------------------
 * Engine level: VideoAligner (alignment.hpp:51-99) and VideoStabilizer (stabilizer.hpp:32-56)
 * ------------------------------------------------------------------------------------------ */
typedef struct vs_aligner vs_aligner;
/* per-frame detail of the last align call(s), for parity tests and the per-stage report */
typedef struct vs_align_info {
    int32_t status;          /* 1 aligned, 0 not aligned */
    int32_t fail_reason;     /* 0 ok, 1 first frame, 2 max iterations, 3 over displacement */
    int32_t fail_level;
    int32_t levels;
    int32_t iterations[16];
    double  condition[16];
    double  phase_dx, phase_dy, phase_response;   /* cv::phaseCorrelate result of the pair (phase_correlate only, else 0) */
    /* the custom metrics of the reference's PerformanceMetrics (alignment.cpp:489-490 "SelectedPointsX_/Y_<level>") and the
     * estimate each level ended on (centre-based, that level's pixels, before the x2 of TX,TY at :683-687): set for every
     * level the pair reached; a level that ran out of iterations (fail_reason 2) leaves its transform 0 */
    int32_t selected_x[16], selected_y[16];
    vs_transform level_transform[16];
} vs_align_info;

vs_aligner* vs_aligner_create(const vs_aligner_params* params /* NULL = defaults */, int device);
void vs_aligner_destroy(vs_aligner* a);
/* Error protocol of the engine-level calls: a call that returns < 0 (a refused allocation: VS_ERR_HIP, an unsupported size, ...)
 * leaves the handle consistent and usable -- no buffer is lost or freed twice -- and ENDS the running sequence: the next frame
 * is the first frame of a new sequence, exactly what a fresh handle would make of it.  (The reference: a failed kernel call
 * returns false and sets LastWidth = -1, so the next AlignNextFrame re-initialises, alignment.cpp:357-367.) */
/* New handles start in VS_SELECT_DEVICE, or in the mode the environment variable VS_SELECT_MODE=0|1|2 names (read once per
 * process, reported once on stderr when it takes effect: the modes differ in the last bits of the transforms); set_select_mode
 * overrides either.  vs_aligner_get_select_mode returns the mode in force (or VS_ERR_ARG). */
int  vs_aligner_set_select_mode(vs_aligner* a, int select_mode);
int  vs_aligner_get_select_mode(const vs_aligner* a);
/* Which build of the per-pair solver kernel a batch (>= 32 frame pairs, levels of <= 26000 tiles) runs through.  The
 * results are bit-identical either way.
 *   VS_BATCH_EXCLUSIVE (default)  one 512-thread workgroup per pair, a whole CU each: fastest when nothing else is running.
 *   VS_BATCH_SHARED               the small-footprint build (256 threads, <= 128 VGPRs, <= 36 KB LDS: the footprint of one
 *                                 bgr_image_warp workgroup; levels whose selection arrays do not fit select on global scratch).  For callers that keep the GPU busy on another stream while the
 *                                 alignment runs -- typically the warp of the previous clip (stabilizer.cpp:97-99 after
 *                                 :19): the pairs move into CUs as the other grid's workgroups retire instead of waiting
 *                                 for whole CUs to drain. */
enum { VS_BATCH_EXCLUSIVE = 0, VS_BATCH_SHARED = 1 };
int  vs_aligner_set_batch_mode(vs_aligner* a, int batch_mode);
/* forget the sequence: the next frame is treated as the first frame of a new clip (device memory is kept) */
int  vs_aligner_reset(vs_aligner* a);
/* Stream ordering of the engine-level calls.  A handle works on its own non-blocking stream (vs_aligner_stream), which
 * is NOT ordered against the caller's streams, the NULL stream included.  With VS_MEM_DEVICE the frames must therefore be
 * complete before an align / process call -- either the producer stream has been synchronised, or
 * vs_aligner_wait_stream(a, producer_stream) was called after the last producer enqueue: everything enqueued on
 * producer_stream up to that point then happens before whatever the handle enqueues afterwards.  In the other direction
 * nothing is needed: align / process calls return after their device work has finished (they hand results to the host). */
void* vs_aligner_stream(const vs_aligner* a);
int   vs_aligner_wait_stream(vs_aligner* a, void* producer_stream);
/* VideoAligner::AlignNextFrame (alignment.hpp:55-58, alignment.cpp:334-704).
 * returns 1 aligned / 0 not aligned (first frame, no convergence, over displacement) / <0 error.  When not aligned,
 * *out holds what the reference leaves in `transform`: identity for the first frame, else the estimate reached when the
 * level gave up (VideoStabilizer passes it on to the smoother regardless, stabilizer.cpp:18-44).
 * `params` may change per call like the reference's third argument (NULL = the creation params). */
int  vs_aligner_align_next(vs_aligner* a, const void* frame, int w, int h, int stride, int format, int mem,
                           const vs_aligner_params* params, vs_transform* out);
/* Batched form: exactly the results of n successive vs_aligner_align_next calls on this handle
 * (state carries over between calls), but every stage runs as one launch over all frames /
 * frame pairs.  frames: n frames, frame i at frames + i*frame_stride (elements).  out[n],
 * status[n] (1/0 per frame).  Returns the number of aligned frames, or <0 on error. */
int  vs_aligner_align_batch(vs_aligner* a, const void* frames, size_t frame_stride, int n,
                            int w, int h, int stride, int format, int mem,
                            const vs_aligner_params* params, vs_transform* out, int32_t* status);
/* Many independent clips at once: n_clips clips of frames_per_clip frames, back to back (clip c, frame k at index
 * c*frames_per_clip + k).  Results = every clip aligned by its own fresh VideoAligner (frame 0 of each clip: status 0,
 * fail_reason 1), computed together so that short clips still fill the GPU.  Resets the handle's running sequence. */
int  vs_aligner_align_clips(vs_aligner* a, const void* frames, size_t frame_stride, int n_clips, int frames_per_clip,
                            int w, int h, int stride, int format, int mem,
                            const vs_aligner_params* params, vs_transform* out, int32_t* status);
/* detail for frame i of the most recent align_next (i = 0) / align_batch call */
int  vs_aligner_get_info(const vs_aligner* a, int i, vs_align_info* info);
/* device pointers / dims of internal per-level state of the most recent call (parity tests) */
int  vs_aligner_level_dims(const vs_aligner* a, int level, int* w, int* h, int* tiles_x, int* tiles_y, int* tile_size);
/* copies out (to host) level images / keypoint tables of frame i of the most recent call */
int  vs_aligner_read_level_image(const vs_aligner* a, int i, int level, uint8_t* out);
int  vs_aligner_read_level_argmax(const vs_aligner* a, int i, int level, int set, uint16_t* out);
int  vs_aligner_read_level_jacobian(const vs_aligner* a, int i, int level, int set, float* out);

/* Opt-in per-stage timing (the reference's compiled-out PerformanceMetrics / TIME_FUNCTION,
 * alignment.cpp:10-147).  Device stages are bracketed with hipEvents on the handle's stream, the
 * selection stage is host wall-clock.  Values accumulate until reset. */
enum {
    VS_STAGE_INGEST = 0,     /* H2D (host frames) + BGR->gray / gray copy   "ConvertToBGR"       */
    VS_STAGE_PYR_DOWN = 1,   /* all pyr_down launches                       "PyrDown_i"          */
    VS_STAGE_KEYFRAME = 2,   /* fused grad/argmax/jacobian launches         "GradXY_i".."SparseJacobian_i" */
    VS_STAGE_WARPDIFF = 3,   /*                                             "SparseWarpDiff_X/Y_i" */
    VS_STAGE_SELECT = 4,     /* keep-best-80% incl. its copies              "NthElement_i"       */
    VS_STAGE_GATHER = 5,     /*                                             "JacobianSetup_i"    */
    VS_STAGE_GN = 6,         /* Hessian + solve + all iterations            "ICAIteration_i_iter" */
    VS_STAGE_PHASE = 7,      /* level-2 spectra + cross-power/inverse/peak  "PhaseCorrelation"   */
    VS_STAGE_COUNT = 8
};
typedef struct vs_stage_timings {
    double ms[VS_STAGE_COUNT];        /* accumulated milliseconds per stage */
    int64_t launches[VS_STAGE_COUNT]; /* kernel launches per stage */
    int64_t frames;                   /* frames processed while timing was on */
    int64_t gn_iterations;            /* Gauss-Newton iterations summed over pairs and levels */
} vs_stage_timings;
int  vs_aligner_enable_timing(vs_aligner* a, int enable);   /* also resets the accumulators */
int  vs_aligner_get_timings(vs_aligner* a, vs_stage_timings* out);

typedef struct vs_stabilizer vs_stabilizer;
vs_stabilizer* vs_stabilizer_create(const vs_stabilizer_params* params /* NULL = defaults */, int device);
void vs_stabilizer_destroy(vs_stabilizer* s);
/* VideoStabilizer::processFrame (stabilizer.hpp:39, stabilizer.cpp:9-117).  frame: interleaved BGR
 * u8 (VS_FMT_BGR8) or u16 (VS_FMT_BGR10 / BGR12 / BGR16_FULL).  out: (w-2*crop)*(h-2*crop)*3 elements, dense.
 * returns 1 when an output frame was written (0 for the first `lag` frames), <0 on error. */
int  vs_stabilizer_process(vs_stabilizer* s, const void* frame, int w, int h, int stride, int format, int mem,
                           void* out, int* out_w, int* out_h);
/* Batched form: exactly n successive vs_stabilizer_process calls (one batched alignment, the reference's scalar
 * bookkeeping in order on the host, batched warps).  frames: frame i at frames + i*frame_stride (elements);
 * has_output[i] = 1 when input frame i produced an output, written dense at out + i*out_frame_stride (elements,
 * >= out_w*out_h*3).  Returns the number of output frames, or <0. */
int  vs_stabilizer_process_batch(vs_stabilizer* s, const void* frames, size_t frame_stride, int n, int w, int h, int stride,
                                 int format, int mem, void* out, size_t out_frame_stride, int32_t* has_output,
                                 int* out_w, int* out_h);
/* The batched form on YCbCr frames (the descriptor and the rule: see vs_ycbcr_to_bgr_batch).  The result is, bit for bit,
 * vs_ycbcr_to_bgr_batch(frames) -> vs_stabilizer_process_batch -> vs_bgr_to_ycbcr_batch of the frames that have an output: output frame i
 * goes to index i of `out`, at out_w x out_h; `out` carries its own subsampling and layout; planes of frames without an output are not
 * written.  A wrapper, not another engine: the planes are converted into a BGR buffer the handle keeps, the batch call runs on it in
 * device memory, ordered on the handle's stream, and every contiguous run of output frames is converted back -- straight into device
 * planes, or through staged spans for host callers.  The handle's two BGR buffers are grown on demand, freed by vs_stabilizer_destroy and
 * never allocated unless this entry point is called: a handle that never calls it is the handle it was.  Every setting (lens, fill,
 * deblur, denoise, rolling shutter, deflicker, inpaint), every error and the state protocol are the inner call's.  A failure before the
 * inner call (an argument, an allocation, the conversion) leaves the stabilizer's state untouched; one behind it ends the running
 * sequence like a failure of the inner call itself, and the handle stays usable.  Returns the number of output frames, or <0. */
int  vs_stabilizer_process_batch_ycbcr(vs_stabilizer* s, const vs_ycbcr_planes* frames, int n, int w, int h, int format, int mem,
                                       const vs_ycbcr_planes* out, int32_t* has_output, int* out_w, int* out_h);
/* Many independent clips at once: n_clips clips of frames_per_clip frames back to back (clip c, frame k at index
 * c*frames_per_clip + k, outputs at the same index).  Results = every clip through its own fresh VideoStabilizer, with the
 * alignment and the warps of all clips batched together.  The handle is reset before the first and after the last clip. */
int  vs_stabilizer_process_clips(vs_stabilizer* s, const void* frames, size_t frame_stride, int n_clips, int frames_per_clip,
                                 int w, int h, int stride, int format, int mem, void* out, size_t out_frame_stride,
                                 int32_t* has_output, int* out_w, int* out_h);
int  vs_stabilizer_reset(vs_stabilizer* s);   /* start a new clip; device buffers are kept */
/* stream ordering for VS_MEM_DEVICE frames: see vs_aligner_wait_stream */
void* vs_stabilizer_stream(const vs_stabilizer* s);
int   vs_stabilizer_wait_stream(vs_stabilizer* s, void* producer_stream);
/* the selection rule of the stabilizer's aligner (VS_SELECT_*, see vs_aligner_set_select_mode); takes effect with the next frame */
int   vs_stabilizer_set_select_mode(vs_stabilizer* s, int mode);
int   vs_stabilizer_get_select_mode(const vs_stabilizer* s);
/* Border fill (the rule: see the fill_batch warp call).  0 (default): off.  1 .. lag: the pixels of every output frame that
 * the corrected frame does not cover are filled from the next `ahead` input frames -- they are already held in device memory
 * and their measured motions are known, so the fill costs no latency and no second alignment.  A frame whose alignment failed
 * ends the list at that frame; frames beyond a reset, a clip boundary or a size change are never candidates.  Takes effect
 * with the next output frame.  VS_ERR_ARG beyond the handle's lag; a handle whose warp_mode is not VS_WARP_BILINEAR_CV
 * returns VS_ERR_UNSUPPORTED.  With the fill on, crop_pixels may go to 0. */
int   vs_stabilizer_set_border_fill(vs_stabilizer* s, int ahead);
int   vs_stabilizer_get_border_fill(const vs_stabilizer* s);
/* The border fill's seam blend (the rule: see vs_bgr_image_warp_fill_blend_batch).  NULL or {0, 0} (default): off -- the fill as
 * it is without this call, launch for launch.  feather 1 .. 6: the fill is cross-faded into the frame's own pixels over 2^feather
 * source pixels inside the edge of its coverage.  match 1: every fill candidate is scaled per channel to the output frame's
 * exposure; the channel sums of every arriving frame are then computed on the device at ingest (always of the ORIGINAL input
 * frames, also when deblur or denoise replaces candidate 0's pixels) and never reach the host.  Meaningful only while the border
 * fill is on; takes effect with the next output frame -- switching match on mid-clip gives what a handle that had it from the
 * first frame gives (the sums of the frames already queued are computed at the next call).  A handle whose warp_mode is not
 * VS_WARP_BILINEAR_CV returns VS_ERR_UNSUPPORTED. */
int   vs_stabilizer_set_fill_blend(vs_stabilizer* s, const vs_fill_blend_params* params);
int   vs_stabilizer_get_fill_blend(const vs_stabilizer* s, vs_fill_blend_params* params);
/* Deblur (the rule: see vs_bgr_deblur_batch).  0 (default): off.  1 .. lag: every frame is deblurred from the next `ahead` input
 * frames before it is warped -- they are already held in device memory with their measured motions, and their sharpness was
 * computed on the device when they arrived, so the pass costs no latency, no second alignment and no host synchronisation.
 * Candidate j's transform is inverse(T_{k+1} o .. o T_j); a frame whose alignment failed ends the list, frames beyond a reset,
 * a clip boundary or a size change are never candidates.  Every warp_mode: the pass only replaces the warp's source (with
 * the border fill on too, the fill's candidate 0 is the deblurred frame, its other candidates the original frames).  The aligner
 * always sees the original frames: transforms, vs_stabilizer_state and has_output do not depend on this setting.  params: NULL =
 * defaults.  Takes effect with the next output frame.  VS_ERR_ARG beyond the handle's lag.  get returns `ahead`. */
int   vs_stabilizer_set_deblur(vs_stabilizer* s, int ahead, const vs_deblur_params* params);
int   vs_stabilizer_get_deblur(const vs_stabilizer* s);
/* Temporal denoise (the rule: see vs_bgr_denoise_batch).  0 (default): off.  1 .. lag: every frame is averaged, pixel by pixel, with what
 * the next `ahead` input frames show at the same scene point, before it is warped -- they are already held in device memory with their
 * measured motions, so the pass costs no latency, no second alignment and no host synchronisation.  Candidate j's transform is
 * inverse(T_{k+1} o .. o T_j); a frame whose alignment failed ends the list, frames beyond a reset, a clip boundary or a size change are
 * never candidates.  Order: deblur (if on), denoise, warp, border fill (if on).  The target is the deblurred frame when deblur is on; the
 * candidates are always the original input frames; every warp_mode reads the denoised frame; the fill's candidate 0 is the denoised frame
 * and its other candidates stay the originals.  The aligner always sees the original frames: transforms, vs_stabilizer_state and
 * has_output do not depend on this setting.  params: NULL = defaults.  Takes effect with the next output frame.  VS_ERR_ARG beyond the
 * handle's lag or for a strength outside 1 .. 255.  get returns `ahead`. */
int   vs_stabilizer_set_denoise(vs_stabilizer* s, int ahead, const vs_denoise_params* params);
int   vs_stabilizer_get_denoise(const vs_stabilizer* s);
/* Rolling-shutter correction (the rule: see vs_bgr_rolling_batch).  NULL or readout == 0 (default): off -- the handle as it is without this
 * call, launch for launch, and no scratch.  Otherwise every frame is corrected, before it is warped, by the motion the aligner measured to
 * the input frame that follows it (candidate 1's transform of the look-ahead lists, inverse(T_{k+1})): no latency, no second alignment, no
 * host synchronisation, one scratch frame per output frame of the call.  A failed alignment of the following frame, or lag == 0, means no
 * motion: the frame passes bit for bit.  Order: deblur, denoise, rolling shutter, warp, border fill, inpaint, gain pass.  The frame
 * corrected is the one deblur and denoise leave; the warp (every warp_mode), the fill's candidate 0 and the coverage index take the
 * corrected frame; the fill's other candidates and the deblur's, denoise's and deflicker's samples stay the raw input frames.  The aligner
 * always sees the original frames: transforms, vs_stabilizer_state and has_output do not depend on this setting.  Takes effect with the
 * next output frame.  VS_ERR_ARG for a readout that is NaN or outside -1 .. 1.  get: the parameters in force (readout 0: off). */
int   vs_stabilizer_set_rolling_shutter(vs_stabilizer* s, const vs_rolling_params* params);
int   vs_stabilizer_get_rolling_shutter(const vs_stabilizer* s, vs_rolling_params* params);
/* Lens-distortion correction (the map: see vs_lens_map; the sample rule: see vs_bgr_remap_batch).  NULL params, or all eight coefficients 0
 * with zoom 1 (the identity lens): off -- the handle as it is without this call, launch for launch, allocation for allocation.  Otherwise
 * every arriving w x h frame is remapped through the lens map, under params->border, IN FRONT OF EVERYTHING: the aligner, the sharpness and
 * channel-sum measurements, the queue and every pass see corrected frames.  The definition: a handle with the correction on, fed raw frames,
 * returns bit for bit -- outputs, has_output, vs_stabilizer_state -- what a handle with it off returns when fed
 * vs_bgr_remap_batch(raw, vs_lens_map(params)).  The map is made once per (params, w, h) on the device, kept in the handle and dropped by
 * this call.  While the pass is on, frames of another size are VS_ERR_ARG before any work.  Device frames are read in place by the remap;
 * host frames are staged first.  Dense device-resident batches take the plain route while the pass is on: the warps do not run under the
 * next sub-batch's alignment.  Takes effect with the next frame; frames already queued stay as they arrived.  VS_ERR_ARG for parameters
 * vs_lens_map refuses or a border other than VS_BORDER_*.  get: returns 1 (on: the parameters and the size in force) or 0 (off: the
 * identity lens, size 0 x 0). */
int   vs_stabilizer_set_lens(vs_stabilizer* s, const vs_lens_params* params, int w, int h);
int   vs_stabilizer_get_lens(const vs_stabilizer* s, vs_lens_params* params, int* w, int* h);
/* Deflicker (the rule: see vs_bgr_exposure_stats_batch).  0 (default): off -- the handle as it is without this call, launch for launch.
 * 1 .. lag: every output frame's exposure is pulled to the average exposure of itself and the next `ahead` input frames; the exposure
 * ratios are measured on the device at the same scene points through the measured motions (candidate j's transform is
 * inverse(T_{k+1} o .. o T_j), as in the denoise), always between the ORIGINAL input frames, and never reach the host.  A frame whose
 * alignment failed ends the list; frames beyond a reset, a clip boundary or a size change are never candidates.  Order: deblur,
 * denoise, warp, border fill (with or without blend), then the gain pass, last, in place on the output window, for every warp_mode.
 * The aligner always sees the original frames: transforms, vs_stabilizer_state and has_output do not depend on this setting.  params:
 * NULL = defaults.  Takes effect with the next output frame.  VS_ERR_ARG beyond the handle's lag or for a step outside 1 .. 64.  get
 * returns `ahead`. */
int   vs_stabilizer_set_deflicker(vs_stabilizer* s, int ahead, const vs_deflicker_params* params);
int   vs_stabilizer_get_deflicker(const vs_stabilizer* s);
/* Inpaint (the rule: see vs_bgr_fill_coverage_batch).  0 (default): off -- the handle as it is without this call, launch for launch.
 * 1: what neither the frame itself nor a fill candidate covers in the output window is inpainted from the window's covered pixels, so
 * that crop_pixels 0 leaves no border colour behind.  Works with the border fill on or off (off: the list is candidate 0 alone).
 * Order: deblur, denoise, warp, border fill (with or without blend), coverage index from the fill's candidate list, inpaint in place
 * on the output window, then the deflicker's gain pass, last.  A run of frames whose own source covers the whole window -- every frame
 * at the default crop -- launches nothing for this pass.  VS_ERR_UNSUPPORTED on a handle with another warp_mode than
 * VS_WARP_BILINEAR_CV; VS_ERR_ARG for a value other than 0 or 1.  Takes effect with the next output frame.  get returns the switch. */
int   vs_stabilizer_set_inpaint(vs_stabilizer* s, int on);
int   vs_stabilizer_get_inpaint(const vs_stabilizer* s);
/* Scene-cut detection (the rule: see vs_bgr_scene_stats_batch).  NULL (default): off -- the handle as it is without this call, launch for
 * launch and allocation for allocation.  On: every arriving frame that has a predecessor in the same clip is compared with it through the
 * motion the aligner has just measured (one statistics launch and one download of two words per frame and call).  A frame whose pair is a
 * cut (a) enters the smoother and the queue with the identity as its measurement, (b) counts as a failed alignment for every look-ahead
 * pass: border fill, fill blend, deblur, denoise, deflicker, rolling shutter and the inpaint's coverage all end their candidate lists in
 * front of it, so nothing of the new scene reaches the old one's frames, (c) leaves the accumulated correction alone on arrival (the
 * frames of the old scene that are still queued finish as they would have) and, when it is itself finalised, gets the identity as its
 * correction and resets the accumulated correction: the new scene starts from a clean path.  vs_stabilizer_state reports the identity and
 * last_success == 0 for a cut frame.  With the lens correction on the statistic sees corrected frames.  vs_stabilizer_reset, a size or
 * format change and every clip start of vs_stabilizer_process_clips forget the predecessor and the cut list.  Takes effect with the next
 * frame.  Not detected: fades and dissolves; a flash frame is two cuts; an exposure jump above about 25 % at mid-grey crosses the default
 * threshold.  VS_ERR_ARG for a step outside 1 .. 64 or a threshold outside 1 .. 255.
 * get_scene_cut: returns 1 (on: *params in force) or 0 (off: *params = the defaults).
 * get_scene_cuts: returns the number of cuts since the last reset and writes, in ascending order, the 0-based indices (counted from that
 * reset) of the most recent min(total, cap, 256) cut frames; frames may be NULL with cap == 0. */
int   vs_stabilizer_set_scene_cut(vs_stabilizer* s, const vs_scene_params* params /* NULL = off */);
int   vs_stabilizer_get_scene_cut(const vs_stabilizer* s, vs_scene_params* params);
int   vs_stabilizer_get_scene_cuts(const vs_stabilizer* s, int64_t* frames, int cap);
/* Phase-compensated sharpening (the rule: see vs_bgr_sharpen_batch).  NULL (default): off -- the handle as it is without this call, launch
 * for launch and allocation for allocation.  On: the warp -- with fill, blend and inpaint as configured -- writes groups of output windows
 * into a scratch buffer of the handle (one allocation, at most 256 MB or one window), and the sharpen writes them to where they went
 * before, each under its own frame's correction; the deflicker's gain follows in place as before.  Fill and inpaint pixels and their edge
 * neighbours are not sharpened, nor is the window's outer ring.  A frame whose correction puts every pixel on phase 0 comes back bit for
 * bit; its launch is not skipped.  VS_ERR_UNSUPPORTED on a handle with another warp_mode than VS_WARP_BILINEAR_CV; VS_ERR_ARG for a
 * strength outside 1 .. 32.  Takes effect with the next output frame.
 * get_sharpen: returns 1 (on: *params in force) or 0 (off: *params = the defaults). */
int   vs_stabilizer_set_sharpen(vs_stabilizer* s, const vs_sharpen_params* params /* NULL = off */);
int   vs_stabilizer_get_sharpen(const vs_stabilizer* s, vs_sharpen_params* params);
/* Output size (the rule: THE RESIZE RULE, see vs_bgr_resize_batch).  (0, 0) (default): off -- the crop window (w - 2 crop) x (h - 2 crop) is
 * delivered, and the handle is the one it is without this call, launch for launch and allocation for allocation.  (-1, -1): every frame is
 * delivered at the source frame's size ("zoom to fill").  (dw, dh), each 1 .. 32767: that size.  On: the warp -- with fill, inpaint,
 * sharpen and the deflicker's gain as configured -- writes groups of output windows into a scratch buffer of the handle (one allocation, at
 * most 256 MB or one window), and the resize, last on the run's stream, writes the delivered frames to where the windows went before:
 * what a handle with the pass off returns, put through vs_bgr_resize_batch, bit for bit.  out_w, out_h, out_frame_stride and the output
 * planes of vs_stabilizer_process_batch_ycbcr then take the delivered size.  A call whose window already has the requested size launches
 * and allocates nothing for this pass.  A call whose window VS_RESIZE_AREA cannot take to the size (delivered <= window <= 8 delivered on
 * each axis) returns VS_ERR_UNSUPPORTED before any work and leaves the handle's state as it was; so does set_output_size for a size above
 * 32767.  VS_ERR_ARG for another filter or any other pair of sizes.  Takes effect with the next call.
 * get_output_size: the three values as set; returns 1 (a size is set) or 0 (off). */
int   vs_stabilizer_set_output_size(vs_stabilizer* s, int dw, int dh, int filter /* VS_RESIZE_* */);
int   vs_stabilizer_get_output_size(const vs_stabilizer* s, int* dw, int* dh, int* filter);
void vs_stabilizer_state(const vs_stabilizer* s, vs_transform* last_meas, vs_transform* accum, int* last_success);

#ifdef __cplusplus
}
#endif
#endif
