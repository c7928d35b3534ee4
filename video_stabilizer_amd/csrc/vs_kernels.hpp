// vs_kernels.hpp -- host-callable launchers of the gfx950 kernels (all async on `s`).
// Batched launchers take frame strides in ELEMENTS and a frame count in grid.z / grid.y.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct vs_lens_params;      // include/vs_amd.h
struct vs_ycbcr_planes;

namespace vsk {

// output window of a warp: output pixel (x, y), x < w, y < h, is pixel (x + Roi.x, y + Roi.y) of the full output frame
struct Roi { int x, y, w, h; };

hipError_t calib_copy12(const void* src, void* dst, size_t bytes, hipStream_t s);

hipError_t pyr_down(const uint8_t* in, int w, int h, int in_stride, uint8_t* out, int ow, int oh, int out_stride,
                    int n_frames, size_t in_frame_stride, size_t out_frame_stride, hipStream_t s);
hipError_t bgr_to_gray(const void* src, int w, int h, int src_stride, int bits, int shift_to_8, uint8_t* dst,
                       int dst_stride, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, hipStream_t s);
// BGR -> gray level 0 (dense, stride w) and level 1 (dense, stride w/2) of every frame's pyramid in one pass
hipError_t ingest_pyr(const void* src, int w, int h, int src_stride, int bits, int shift_to_8, uint8_t* g0, uint8_t* g1,
                      int n_frames, size_t src_frame_stride, size_t pyr_frame_stride, hipStream_t s);
hipError_t grad_xy(const uint8_t* in, int w, int h, int stride, float* gx, float* gy, hipStream_t s);
hipError_t grad_argmax(const float* gx, const float* gy, int w, int h, int ts, uint16_t* lmx, uint16_t* lmy,
                       hipStream_t s);
hipError_t sparse_jac(const float* gx, const float* gy, int w, int h, const uint16_t* lmx, const uint16_t* lmy, int nt,
                      float* jx, float* jy, hipStream_t s);
hipError_t keyframe(const uint8_t* img, int w, int h, int stride, int ts, uint16_t* lmx, uint16_t* lmy, float* jx,
                    float* jy, int n_frames, size_t img_frame_stride, size_t lm_frame_stride, size_t jac_frame_stride,
                    hipStream_t s, bool aos = false);   // aos: the engine's table layout ({x, y} pairs, float4 Jacobians), see vs_engine.hip
// every pyramid level of n_frames keyframes in ONE launch: pyr / lm / jac = slot of the first keyframe, levels at the given
// element offsets inside a slot (x-set table at lm_off, y-set 2*nt later; x-set Jacobians at jac_off, y-set 4*nt later);
// always the engine's layout: {x, y} pairs and float4 Jacobians per tile
struct KeyframeLevel { int w, h, ts, tx, ty, strips_x, blocks; size_t img_off, lm_off, jac_off; };
struct KeyframeLevels { int n; KeyframeLevel lv[16]; };
bool keyframe_levels_supported(const KeyframeLevels& L);
hipError_t keyframe_levels(const uint8_t* pyr, uint16_t* lm, float* jac, KeyframeLevels L, int n_frames, size_t pyr_frame_stride,
                           size_t lm_frame_stride, size_t jac_frame_stride, hipStream_t s);
hipError_t sparse_warpdiff(const uint8_t* tmpl, const uint8_t* key, int w, int h, int stride, const uint16_t* lm,
                           int nt, float A, float B, float TX, float TY, uint16_t* out, hipStream_t s);
hipError_t sparse_ica(const uint8_t* tmpl, const uint8_t* key, int w, int h, int stride, const uint16_t* selx, int nx,
                      const uint16_t* sely, int ny, const float* jacx, const float* jacy, float A, float B, float TX,
                      float TY, double* out, hipStream_t s);
hipError_t image_warp(const uint8_t* in, int w, int h, int stride, float A, float B, float TX, float TY, float* out,
                      int ow, int oh, hipStream_t s);
// params_dev: n_frames float4 {A,B,TX,TY} (upper-left based kernel arguments) in device memory
hipError_t bgr_warp_generic(const void* src, int w, int h, int src_stride, int channels, int bits,
                            const float4* params_dev, int mode, int border, int max_value, void* dst, int dst_stride,
                            bool f32out, int n_frames, size_t src_frame_stride, size_t dst_frame_stride, Roi roi, hipStream_t s);
// tuned interleaved 3-channel path, u8 or u16 (vs_warp.hip); hipErrorNotSupported when the grid would overflow
// compact: 0 the standard window; 1 / 2: every frame fits the 20-row windows of the contracted / separable forms' six- / seven-wave instantiations (bgr_warp_c3_compact_shape on the extents)
// tab_dev: device scratch of n_frames * bgr_warp_c3_table_bytes(bits, mode, roi) bytes (16-byte aligned) or null -- the float-tile Lanczos2 forms' per-launch
// tables (tile windows, row position terms), written by a small kernel in front of the warp launch on the same stream; read only together with the extents
hipError_t bgr_warp_c3(const void* src, int w, int h, int src_stride, int bits, const float4* params_dev, const float4* extents_dev, void* tab_dev,
                       int mode, int border, int max_value, void* dst, int dst_stride, int n_frames, size_t src_fs, size_t dst_fs, Roi roi,
                       int compact, hipStream_t s);
size_t bgr_warp_c3_table_bytes(int bits, int mode, Roi roi);
int bgr_warp_c3_compact_shape(const float* E4, int n_frames);
// VS_WARP_BILINEAR_CV (cv::warpAffine's fixed-point bilinear): minv_dev = n_frames x 6 doubles, the output -> source matrix of each frame
// (vs_cv_inverse_matrix).  Generic: any channel count, u8 / u16 containers; tuned (vs_warp.hip): interleaved 8-bit BGR saturating at 255,
// hipErrorNotSupported for anything else
hipError_t bgr_warp_cv_generic(const void* src, int w, int h, int src_stride, int channels, int bits, const double* minv_dev, int border,
                               int max_value, void* dst, int dst_stride, int n_frames, size_t src_fs, size_t dst_fs, Roi roi, hipStream_t s);
// (tuned) tab_dev: device scratch of n_frames * bgr_warp_cv_table_ints(bits, roi) ints -- the per-frame coordinate tables, written by a small
// kernel in front of the warp launch on the same stream (cv::warpAffine's adelta / bdelta / row origins, made once per frame as OpenCV makes them)
// minv_host (n_frames x 6 doubles on the host) may stand in for minv_dev when n_frames <= kCvInlineFrames: the matrices then travel as kernel arguments
size_t bgr_warp_cv_table_ints(int bits, Roi roi);
constexpr int kCvInlineFrames = 64;          // 3 KiB of kernel arguments
hipError_t bgr_warp_cv_c3(const void* src, int w, int h, int src_stride, int bits, const double* minv_dev, const double* minv_host, int* tab_dev, int border, int max_value,
                          void* dst, int dst_stride, int n_frames, size_t src_fs, size_t dst_fs, Roi roi, hipStream_t s);
// Border fill behind a VS_WARP_BILINEAR_CV warp (vs_fill.hip: the rule and the kernel): the pixels of output frame o that its own source does not
// cover are rewritten from the first of its candidates 1 .. n_cand-1 that covers them.  cands_dev: n_frames x n_cand entries in device memory;
// entry 0 of a frame carries the matrix pass 1 warped it with (its frame pointer is not read), a null frame ends the list.  3 channels,
// frames up to 32767 a side; hipErrorNotSupported otherwise.  Same stream as the warp, after it.
struct FillCand { double m[6]; const void* src; unsigned long long reserved; };      // 64 bytes = four float4 slots of the parameter ring
hipError_t bgr_warp_cv_fill_c3(const FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int max_value, void* dst, int dst_stride,
                               int n_frames, size_t dst_fs, Roi roi, hipStream_t s);
// The fill with its seams blended (vs_fill.hip, THE BLEND RULE): feather 0 .. 6, match: gain matching from whole-frame channel sums.  With match
// every entry arrives with `reserved` = where the three sums of its frame lie in device memory (entry 0: the output frame's) and a small kernel in
// front turns them into packed Q15 gains; without it the entries c >= 1 carry fill_unit_gains().  cands_dev is written (the gains), so it is
// not const.  bgr_channel_sums: out[3 i + c] (device) = the sum of channel c's samples of frame i; zeroes `out` on `s` first.
unsigned long long fill_unit_gains();
hipError_t bgr_channel_sums(const void* src, int w, int h, int src_stride, int bits, unsigned long long* out, int n_frames, size_t src_fs, hipStream_t s);
hipError_t bgr_warp_cv_fill_blend_c3(FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int max_value, int feather, bool match, void* dst,
                                     int dst_stride, int n_frames, size_t dst_fs, Roi roi, hipStream_t s);
// Deblur by transfer from sharper frames (vs_deblur.hip: the rule and the kernels).
// bgr_sharpness: out[i] (device, n_frames x uint64) = the gradient energy S of frame i; zeroes `out` on `s` first.
// bgr_deblur: cands_dev = n_frames x n_cand entries in device memory; entry 0 of a frame is the target (frame and sharpness; matrix not read), a
// null frame ends the list; `sharp` points at the frame's S in device memory.  r2_dev: n_frames x n_cand floats of device scratch (the ratios,
// made by a small kernel in front of the deblur launch).  dst: full w x h frames.  targets_aligned: every target frame starts on a dword.
struct DeblurCand { double m[6]; const void* src; const unsigned long long* sharp; };  // 64 bytes = four float4 slots of the parameter ring
hipError_t bgr_sharpness(const void* src, int w, int h, int src_stride, int bits, int shift_to_8, unsigned long long* out, int n_frames, size_t src_fs,
                         hipStream_t s);
hipError_t bgr_deblur(const DeblurCand* cands_dev, float* r2_dev, int n_cand, int w, int h, int src_stride, int bits, int shift_to_8, int max_value,
                      float sensitivity, float max_ratio, void* dst, int dst_stride, int n_frames, size_t dst_fs, bool targets_aligned, hipStream_t s);
// Motion-compensated temporal denoise (vs_denoise.hip: the rule and the kernels).  cands_dev = n_frames x n_cand entries in device memory; entry 0
// of a frame is the target (its matrix is not read), a null frame ends the list.  dst: full w x h frames.  strength: 1 .. 255.  targets_aligned:
// every target frame starts on a dword.
hipError_t bgr_denoise(const FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int shift_to_8, int max_value, int strength, void* dst,
                       int dst_stride, int n_frames, size_t dst_fs, bool targets_aligned, hipStream_t s);
// Rolling-shutter correction (vs_rolling.hip: the rule and the kernel).  cands_dev = n_frames x 2 entries in device memory: entry 0 of a frame
// is the frame to correct (its matrix is not read); entry 1 carries vs_cv_inverse_matrix of the motion to the following frame, and a null frame
// there means "no motion known" (the frame is copied; a non-null one is never followed).  dst: full w x h frames.  readout: -1 .. 1.
hipError_t bgr_rolling(const FillCand* cands_dev, int w, int h, int src_stride, int bits, int max_value, double readout, void* dst, int dst_stride,
                       int n_frames, size_t dst_fs, hipStream_t s);
// Remap through a map of fixed-point positions and the radial lens map (vs_remap.hip: the format, the sample rule and the kernels).  bgr_remap:
// n_frames w x h frames -> n_frames ow x oh frames through ONE map of ow x oh (X, Y) pairs in device memory, rows of map_stride ints; border:
// VS_BORDER_*; slice: how many frames a workgroup takes a pixel through (kRemapSlice unless a measurement says otherwise).  lens_map: the map of
// vs_lens.hpp's rule for a w x h frame.
constexpr int kRemapSlice = 8;
hipError_t bgr_remap(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int bits, int max_value, const int32_t* map,
                     int map_stride, int ow, int oh, int border, void* dst, size_t dst_fs, int dst_stride, int slice, hipStream_t s);
hipError_t lens_map(const vs_lens_params& p, int w, int h, int32_t* map, int map_stride, hipStream_t s);
// YCbCr frames to interleaved BGR and back (vs_ycbcr.hip: the kernels; vs_ycbcr.hpp: the rule).  The descriptor holds device pointers; bits:
// vs_format_bits (8, 10, 12, 16), max_value: vs_format_max_value; w, h in 1 .. 32767 and a descriptor vsy::layout_ok accepts, hipErrorNotSupported
// otherwise.  Four columns per lane with dword accesses where w % 4 == 0 and every row of every plane and of the BGR side starts on a dword,
// one chroma cell per lane otherwise: the same bits.
hipError_t ycbcr_to_bgr(const vs_ycbcr_planes& src, int n_frames, int w, int h, int bits, int max_value, void* dst, size_t dst_fs, int dst_stride, hipStream_t s);
hipError_t bgr_to_ycbcr(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int bits, int max_value, const vs_ycbcr_planes& dst, hipStream_t s);
// Resize by THE RESIZE RULE (vs_resize.hip: the sample rule and the kernels; vs_resize.hpp: the tap tables).  n_frames sw x sh frames -> n_frames
// dw x dh frames; filter: VS_RESIZE_*; tables: resize_table_ints(dw, dh) ints of device scratch, written on `s` in front of the frames' launch
// and read by it.  form: which kernel -- both give the same bits; kResizeAuto: the tiled form where the frame grows in height (dh > sh: destination
// rows share source rows, which the tile forms H of once), the direct form otherwise (measured both ways: DESIGN.md section 30).  A shape
// vsr::resize_params_valid refuses: hipErrorNotSupported.
constexpr int kResizeAuto = -1, kResizeTiled = 0, kResizeDirect = 1;
size_t resize_table_ints(int dw, int dh);
hipError_t bgr_resize(const void* src, size_t src_fs, int n_frames, int sw, int sh, int src_stride, int bits, int max_value, int filter, int* tables,
                      void* dst, size_t dst_fs, int dw, int dh, int dst_stride, int form, hipStream_t s);
// Deflicker (vs_deflicker.hip: the rule and the kernels).  exposure_stats: cands_dev = n_frames x n_cand entries in device memory (entry 0 of a
// frame is the target, a null frame ends the list); stats = n_frames x n_cand x 8 words in device memory, zeroed on `s` first.  exposure_gains:
// gains[4 o + {0..2: G_c, 3: m}] from the statistics.  bgr_gain: frame i scaled by gains[4 i ..] (clamped to 16384 .. 65536); dst may be src.
size_t exposure_threshold(int w, int h, int step);         // max(1, L / 16)
hipError_t exposure_stats(const FillCand* cands_dev, int n_cand, int w, int h, int src_stride, int bits, int shift_to_8, int step, unsigned long long* stats,
                          int n_frames, hipStream_t s);
hipError_t exposure_gains(const unsigned long long* stats, int n_out, int n_cand, int w, int h, int step, uint32_t* gains, hipStream_t s);
hipError_t bgr_gain(const void* src, int w, int h, int src_stride, int bits, int max_value, const uint32_t* gains, void* dst, int dst_stride, int n_frames,
                    size_t src_fs, size_t dst_fs, hipStream_t s);
// Scene-cut detection (vs_scene.hip: the rule and the kernel).  cands_dev = n_pairs x 2 entries in device memory: entry 0 of a pair is the target
// frame (its matrix is not read), entry 1 the candidate frame with vs_cv_inverse_matrix of the pair's transform; a null frame on either side
// leaves the pair's words zero.  stats = n_pairs x 2 words (count, sad) in device memory, zeroed on `s` first.
hipError_t scene_stats(const FillCand* cands_dev, int w, int h, int src_stride, int bits, int shift_to_8, int max_value, int step, unsigned long long* stats,
                       int n_pairs, hipStream_t s);
// Fidelity statistics of image pairs (vs_fidelity.hip: the rule and the kernel).  pairs_dev = n_pairs entries in device memory: image a and image
// b of the pair, both w x h, rows of a_stride / b_stride elements.  on_dwords: every row of every image named starts on a dword (rows_on_dwords of
// both batches).  stats = n_pairs x 6 words (sse_b, sse_g, sse_r, sse_y, n_win, ssim_sum) in device memory, zeroed on `s` first.
struct FidPair { const void* a; const void* b; };                                     // 16 bytes = one float4 slot of the parameter ring
hipError_t bgr_fidelity(const FidPair* pairs_dev, int w, int h, int a_stride, int b_stride, int bits, int shift_to_8, int max_value, bool on_dwords,
                        unsigned long long* stats, int n_pairs, hipStream_t s);
// Phase-compensated sharpening behind VS_WARP_BILINEAR_CV (vs_sharpen.hip: the rule and the kernels).  n_frames images of roi.w x roi.h, the
// window `roi` of w x h output frames; minv_dev = n_frames x 6 doubles in device memory, the output -> source matrix of each frame
// (vs_cv_inverse_matrix); strength: 1 .. 32.  Out of place: src and dst must not overlap.
hipError_t bgr_sharpen(const void* src, size_t src_fs, int n_frames, int w, int h, int src_stride, int bits, int max_value, const double* minv_dev,
                       int strength, Roi roi, void* dst, size_t dst_fs, int dst_stride, hipStream_t s);
// Inpaint of what the fill leaves open (vs_inpaint.hip: the rule and the kernels).  fill_coverage: cands_dev as the fill takes them (entry 0's
// matrix; a null frame ends a list; no frame is read); cov[frame][y * cov_stride + x] = 1 + the first covering candidate, 0 for none;
// open_count (device, may be null): zeroed on `s`, then the frame's number of zeros.  mask_open_count: the same count from a mask.
// bgr_inpaint: n_frames w x h windows in place under their byte masks (non-zero = keep); counts: the frames' open counts in device memory (a
// frame with 0 or w * h is left alone); pyramid: n_frames * inpaint_pyramid_bytes(w, h, bits) bytes of device scratch, 8-byte aligned,
// written before it is read.
hipError_t fill_coverage(const FillCand* cands_dev, int n_cand, int w, int h, uint8_t* cov, int cov_stride, int n_frames, size_t cov_fs, Roi roi,
                         unsigned int* open_count, hipStream_t s);
size_t inpaint_pyramid_bytes(int w, int h, int bits);
hipError_t mask_open_count(const uint8_t* mask, int w, int h, int mask_stride, size_t mask_fs, int n_frames, unsigned int* counts, hipStream_t s);
hipError_t bgr_inpaint(void* img, size_t img_fs, int n_frames, int w, int h, int stride, int bits, const uint8_t* mask, size_t mask_fs, int mask_stride,
                       const unsigned int* counts, void* pyramid, hipStream_t s);
// host side of the tuned kernel's tile prologue: per frame {lo_x, hi_x, lo_y, hi_y} from the kernel parameters {A, B, TX, TY}, for the
// tile of the kernel that bgr_warp_c3 launches for (bits, mode)
void bgr_warp_c3_extents(const float* P4, int n_frames, Roi roi, int bits, int mode, float* E4);

}  // namespace vsk
