// fidelity.hpp -- the harness's picture score: PSNR and SSIM of frame pairs from the library's fidelity statistics (include/vs_amd.h:
// vs_bgr_fidelity_batch, THE FIDELITY RULE).  The jitter scores (jitter.hpp) say how much the camera still moves; nothing there looks at pixel
// values.  The stabilization literature scores a clip by ITF, the inter-frame transformation fidelity: the mean PSNR between consecutive
// frames -- a steady clip's neighbours are alike.  Against a reference clip (a steady twin of a synthetic clip, the clean original of a
// denoise or deblur experiment) the same statistics give PSNR and SSIM frame by frame.
#pragma once
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>
#include "harness.hpp"

namespace vsfid {

// printed once by every tool that reports the score: the score must say what it is where it is read
inline const char* score_note(bool ref) {
    if (ref)
        return "note: psnr_db / psnr_y_db = mean over the frames of min(PSNR, 100) against the same frame of the reference clip, the three channels "
               "pooled / on 8-bit gray; ssim = mean over the frames of the mean integer SSIM of 8 x 8 windows at a stride of 4 on 8-bit gray "
               "(THIS build's specification, include/vs_amd.h: no Gaussian window, constants scaled to 64 samples): values are close to, not "
               "equal to, what other tools print";
    return "note: itf_psnr_db / itf_psnr_y_db = inter-frame transformation fidelity, the mean over consecutive frame pairs of min(PSNR, 100), the "
           "three channels pooled / on 8-bit gray; itf_ssim = the mean over those pairs of the mean integer SSIM of 8 x 8 windows at a stride of 4 "
           "on 8-bit gray (THIS build's specification, include/vs_amd.h: no Gaussian window, constants scaled to 64 samples): values are close "
           "to, not equal to, what other tools print; a pan lowers them like a shake does -- compare clips of one camera path";
}

// the means over the pairs seen so far, summed in the order the pairs come
struct Means {
    double psnr = 0.0, psnr_y = 0.0, ssim = 0.0;
    size_t pairs = 0;
    void add(const vs_fidelity_score& s) {
        psnr += std::min(s.psnr, 100.0);                     // (identical frames: HUGE_VAL)
        psnr_y += std::min(s.psnr_y, 100.0);
        ssim += s.ssim;                                      // (NaN for an image without a window: the mean says so)
        pairs++;
    }
    double mean_psnr() const { return pairs ? psnr / (double)pairs : 0.0; }
    double mean_psnr_y() const { return pairs ? psnr_y / (double)pairs : 0.0; }
    double mean_ssim() const { return pairs ? ssim / (double)pairs : 0.0; }
};

// frames of the default upload chunk: about 256 MiB, 2 .. 64
inline size_t default_chunk(size_t frame_bytes) { return std::min<size_t>(64, std::max<size_t>(2, ((size_t)256 << 20) / std::max<size_t>(frame_bytes, 1))); }

// The mean scores of a clip in host memory.  ref == nullptr: consecutive frames of the clip, pairs (i, i + 1); else frame i of the clip against
// frame i of *ref (same size and depth; the shorter clip ends the comparison).  The image is the frame minus `inset` pixels on every side.  Every
// frame is uploaded once, `chunk` frames at a time; between consecutive frames the last frame of a chunk is carried over to the next on the device.
inline Means measure(const vsio::Clip& clip, const vsio::Clip* ref, int inset, size_t chunk = 0) {
    const int W = clip.fmt.w, H = clip.fmt.h;
    if (ref && (ref->fmt.w != W || ref->fmt.h != H || ref->fmt.bits != clip.fmt.bits))
        throw std::runtime_error("the reference clip is " + std::to_string(ref->fmt.w) + "x" + std::to_string(ref->fmt.h) + " at " + std::to_string(ref->fmt.bits) +
                                 " bits, the clip " + std::to_string(W) + "x" + std::to_string(H) + " at " + std::to_string(clip.fmt.bits));
    if (inset < 0 || 2 * (long long)inset >= W || 2 * (long long)inset >= H) throw std::runtime_error("--inset leaves no image");
    const int w = W - 2 * inset, h = H - 2 * inset, stride = W * 3, format = vsh::vs_format_of(clip.fmt);
    const size_t fe = clip.fmt.bgr_elems(), fb = clip.frame_bytes(), esz = clip.elem_bytes();
    const size_t n = ref ? std::min(clip.frames, ref->frames) : clip.frames;
    chunk = chunk ? std::max<size_t>(2, chunk) : default_chunk(fb);
    const size_t org = ((size_t)inset * (size_t)stride + (size_t)inset * 3) * esz;       // the image's origin inside a frame, in bytes
    Means m;
    vsh::DeviceBuffer da(chunk * fb), db(ref ? chunk * fb : 0), dstats(chunk * 6 * sizeof(uint64_t));
    std::vector<uint64_t> st(chunk * 6);
    std::vector<vs_fidelity_score> sc(chunk);
    std::vector<int32_t> pairs;
    const auto score = [&](const void* b, int frames, int n_pairs) {
        vsh::vs_check(vs_bgr_fidelity_batch((const char*)da.ptr + org, fe, frames, stride, (const char*)b + org, fe, frames, stride, w, h, format, n_pairs,
                                            pairs.data(), (uint64_t*)dstats.ptr, VS_MEM_DEVICE, nullptr), "vs_bgr_fidelity_batch");
        vsh::hip_check(hipMemcpy(st.data(), dstats.ptr, (size_t)n_pairs * 6 * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy D2H");
        vsh::vs_check(vs_fidelity_scores(st.data(), n_pairs, w, h, format, sc.data()), "vs_fidelity_scores");
        for (int i = 0; i < n_pairs; i++) m.add(sc[(size_t)i]);
    };
    if (!ref) {
        size_t have = 0;                                     // frames in the buffer; the last of them is the newest frame uploaded
        for (size_t next = 0; next < n;) {
            if (have > 1) vsh::hip_check(hipMemcpy(da.ptr, (const char*)da.ptr + (have - 1) * fb, fb, hipMemcpyDeviceToDevice), "hipMemcpy D2D");
            have = std::min<size_t>(have, 1);
            const size_t cnt = std::min(chunk - have, n - next);
            vsh::hip_check(hipMemcpy((char*)da.ptr + have * fb, clip.frame(next), cnt * fb, hipMemcpyHostToDevice), "hipMemcpy H2D");
            have += cnt;
            next += cnt;
            if (have < 2) continue;
            pairs.clear();
            for (size_t i = 0; i + 1 < have; i++) { pairs.push_back((int32_t)i); pairs.push_back((int32_t)i + 1); }
            score(da.ptr, (int)have, (int)have - 1);
        }
    } else {
        for (size_t s = 0; s < n; s += chunk) {
            const size_t cnt = std::min(chunk, n - s);
            vsh::hip_check(hipMemcpy(da.ptr, clip.frame(s), cnt * fb, hipMemcpyHostToDevice), "hipMemcpy H2D");
            vsh::hip_check(hipMemcpy(db.ptr, ref->frame(s), cnt * fb, hipMemcpyHostToDevice), "hipMemcpy H2D");
            pairs.clear();
            for (size_t i = 0; i < cnt; i++) { pairs.push_back((int32_t)i); pairs.push_back((int32_t)i); }
            score(db.ptr, (int)cnt, (int)cnt);
        }
    }
    return m;
}

}  // namespace vsfid
