// stabilizer.hpp -- drop-in for the reference's stabilizer.hpp:13-56 on the C ABI.
#pragma once
#include <vector>
#include "alignment.hpp"
#include "smoother.hpp"

// stabilizer.hpp:13-30 -- same fields, same defaults (+ the two sampler knobs of this build)
struct VideoStabilizerParams {
    VideoAlignerParams aligner;
    int lag = 10;
    int smoother_memory = 5;
    double lambda = 4.0;
    bool enable_smoother = true;
    int crop_pixels = 32;
    double min_disp = 48.0, max_disp = 64.0;
    double min_decay = 0.9, max_decay = 0.7;
    int warp_mode = VS_WARP_BILINEAR_CV;  // cv::warpAffine(INTER_LINEAR) as the reference calls it (imgproc.cpp:472), fixed point; VS_WARP_LANCZOS2* = bgr_image_warp
    int warp_border = VS_BORDER_CONSTANT;
    int border_fill = 0;                  // a knob of this build: 1 .. lag = fill what the corrected frame does not cover from that many following frames (vs_stabilizer_set_border_fill)
    int deblur = 0;                       // a knob of this build: 1 .. lag = deblur every frame from the sharper ones among that many following frames (vs_stabilizer_set_deblur, default parameters)
    int denoise = 0;                      // a knob of this build: 1 .. lag = average every frame with what that many following frames show at the same scene point (vs_stabilizer_set_denoise, default parameters)
    int deflicker = 0;                    // a knob of this build: 1 .. lag = pull every frame's exposure to the mean exposure of itself and that many following frames (vs_stabilizer_set_deflicker, default parameters)
    double rolling_shutter = 0.0;         // a knob of this build: the sensor's readout share of the frame period, -1 .. 1, 0 = off; every frame is corrected for its rolling shutter by the motion to the following frame (vs_stabilizer_set_rolling_shutter)
};

// stabilizer.hpp:32-56.  processFrame returns an empty vector until `lag` frames have arrived
// (stabilizer.cpp:46-52), then the stabilized, cropped BGR frame (out_width x out_height x 3).
class VideoStabilizer {
public:
    explicit VideoStabilizer(const VideoStabilizerParams& params = VideoStabilizerParams(), int device = 0) {
        vs_stabilizer_params p;
        vs_stabilizer_params_default(&p);
        p.aligner = params.aligner.c();
        p.lag = params.lag; p.smoother_memory = params.smoother_memory; p.lambda = params.lambda;
        p.enable_smoother = params.enable_smoother ? 1 : 0; p.crop_pixels = params.crop_pixels;
        p.min_disp = params.min_disp; p.max_disp = params.max_disp; p.min_decay = params.min_decay; p.max_decay = params.max_decay;
        p.warp_mode = params.warp_mode; p.warp_border = params.warp_border;
        crop_ = params.crop_pixels > 0 ? params.crop_pixels : 0;
        vs::check_abi();
        h_ = vs_stabilizer_create(&p, device);
        if (!h_) throw std::runtime_error(std::string("vs_stabilizer_create: ") + vs_last_error());
        if (params.border_fill != 0 && vs_stabilizer_set_border_fill(h_, params.border_fill) != VS_OK) {
            const std::string why = vs_last_error();
            vs_stabilizer_destroy(h_);
            throw std::runtime_error("vs_stabilizer_set_border_fill: " + why);
        }
        if (params.deblur != 0 && vs_stabilizer_set_deblur(h_, params.deblur, nullptr) != VS_OK) {
            const std::string why = vs_last_error();
            vs_stabilizer_destroy(h_);
            throw std::runtime_error("vs_stabilizer_set_deblur: " + why);
        }
        if (params.denoise != 0 && vs_stabilizer_set_denoise(h_, params.denoise, nullptr) != VS_OK) {
            const std::string why = vs_last_error();
            vs_stabilizer_destroy(h_);
            throw std::runtime_error("vs_stabilizer_set_denoise: " + why);
        }
        if (params.deflicker != 0 && vs_stabilizer_set_deflicker(h_, params.deflicker, nullptr) != VS_OK) {
            const std::string why = vs_last_error();
            vs_stabilizer_destroy(h_);
            throw std::runtime_error("vs_stabilizer_set_deflicker: " + why);
        }
        if (params.rolling_shutter != 0.0) {
            try { setRollingShutter(params.rolling_shutter); } catch (...) { vs_stabilizer_destroy(h_); throw; }
        }
    }
    // 0: off; else the sensor's readout share of the frame period, -1 .. 1 (negative: bottom-up); takes effect with the next output frame
    void setRollingShutter(double readout) {
        const vs_rolling_params rp{readout};
        if (vs_stabilizer_set_rolling_shutter(h_, &rp) != VS_OK) throw std::runtime_error(std::string("vs_stabilizer_set_rolling_shutter: ") + vs_last_error());
    }
    // nullptr (or the identity lens): off; else every arriving width x height frame is corrected for the lens's distortion in front of everything --
    // the aligner and every pass see corrected frames (vs_stabilizer_set_lens; vs_lens_params_default gives the identity lens to start from)
    void setLens(const vs_lens_params* lens, int width = 0, int height = 0) {
        if (vs_stabilizer_set_lens(h_, lens, width, height) != VS_OK) throw std::runtime_error(std::string("vs_stabilizer_set_lens: ") + vs_last_error());
    }
    ~VideoStabilizer() { vs_stabilizer_destroy(h_); }
    VideoStabilizer(const VideoStabilizer&) = delete;
    VideoStabilizer& operator=(const VideoStabilizer&) = delete;

    std::vector<uint8_t> processFrame(const uint8_t* bgr, int width, int height, int& out_width, int& out_height) {
        std::vector<uint8_t> out((size_t)(width - 2 * crop_) * (height - 2 * crop_) * 3);
        const int r = vs_stabilizer_process(h_, bgr, width, height, width * 3, VS_FMT_BGR8, VS_MEM_HOST, out.data(), &out_width, &out_height);
        if (r < 0) throw std::runtime_error(std::string("vs_stabilizer_process: ") + vs_last_error());
        if (r == 0) { out.clear(); out_width = out_height = 0; }
        return out;
    }
#ifdef VS_FACADE_HAVE_OPENCV
    // stabilizer.hpp:39: an empty cv::Mat until `lag` frames have arrived, then the stabilized, cropped frame
    cv::Mat processFrame(const cv::Mat& inputFrame) {
        vs::require_bgr8(inputFrame, "VideoStabilizer::processFrame");
        cv::Mat out(inputFrame.rows - 2 * crop_, inputFrame.cols - 2 * crop_, CV_8UC3);
        int ow = 0, oh = 0;
        const int r = vs_stabilizer_process(h_, inputFrame.data, inputFrame.cols, inputFrame.rows, vs::mat_stride_elems(inputFrame), VS_FMT_BGR8,
                                            VS_MEM_HOST, out.data, &ow, &oh);
        if (r < 0) throw std::runtime_error(std::string("vs_stabilizer_process: ") + vs_last_error());
        return r == 1 ? out : cv::Mat();
    }
#endif
private:
    vs_stabilizer* h_ = nullptr;
    int crop_ = 0;
};
