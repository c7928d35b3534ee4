// vs_video_test -- stabilize every clip of a directory (the role of the reference's video_test.cpp:10-128).
//   vs_video_test [input_dir=../recordings] [output_dir=output] [--chunk N] [--device D] [--crop N] [--fill N] [--fill-feather N] [--fill-match] [--inpaint] [--deblur N] [--denoise N] [--denoise-strength T] [--deflicker N] [--deflicker-step S] [--scene-cut [T]] [--sharpen [S]] [--rolling-shutter R] [--lens fx,fy,cx,cy,k1,k2,p1,p2[,k3[,k4,k5,k6]]] [--lens-zoom Z] [--bilinear | --lanczos2] [--444] [--device-convert] [--out-size WxH | source] [--out-filter linear|area]
// For each .y4m / .bgr clip writes output_dir/processed_<name>.  Like the reference's driver it runs the default
// VideoStabilizerParams with crop_pixels = 0 (video_test.cpp:54-55) unless --crop is given.  --fill N: what the corrected frame
// does not cover is filled from the next N input frames (vs_stabilizer_set_border_fill); --fill-feather N (1 .. 6) cross-fades the fill into the
// frame's own pixels over 2^N source pixels and --fill-match scales it to the frame's exposure (vs_stabilizer_set_fill_blend).  --inpaint: what
// neither the frame nor a fill candidate covers is inpainted from the window's covered pixels (vs_stabilizer_set_inpaint).  --deblur N: every frame is deblurred from
// the sharper ones among the next N input frames before it is warped (vs_stabilizer_set_deblur).  --denoise N: every frame is averaged
// with what the next N input frames show at the same scene point (vs_stabilizer_set_denoise; --denoise-strength T: 1 .. 255, default 24).  --deflicker N: every
// output frame's exposure is pulled to the mean exposure of itself and the next N input frames (vs_stabilizer_set_deflicker; --deflicker-step S: the lattice
// step of the exposure statistics, 1 .. 64, default 4).  --scene-cut [T]: consecutive frames are compared through their measured motion and a frame that shows
// another scene ends every look-ahead list in front of it and starts a clean path (vs_stabilizer_set_scene_cut; T: the threshold in 8-bit levels, 1 .. 255,
// default 32); the clip's cut list is printed.  --sharpen [S]: every output window is sharpened behind the warp by the sub-pixel phase of its own
// correction, which evens out the bilinear warp's phase-dependent blur (vs_stabilizer_set_sharpen; S: the strength in sixteenths, 1 .. 32, default 16).  --rolling-shutter R: every frame is corrected for a rolling shutter whose readout takes the
// share R (-1 .. 1, negative: bottom-up) of the frame period, by the motion to the following frame (vs_stabilizer_set_rolling_shutter).
// --out-size WxH | source: the crop window is resized to that size, or to the source frame's, behind every other pass and the writer takes that
// size (vs_stabilizer_set_output_size); --out-filter linear|area: the filter, by default area where an axis shrinks by more than 2:1 and linear otherwise.
// --lens fx,fy,cx,cy,k1,k2,p1,p2[,k3[,k4,k5,k6]]: every frame is corrected for that lens's distortion in front of everything (the camera matrix in
// pixels, then OpenCV's distCoeffs in their order; --lens-zoom Z scales the output camera's focal lengths, default 1; vs_stabilizer_set_lens).  Frames go to the GPU in
// chunks of N (default 64) and through vs_stabilizer_process_batch, which is defined as N successive processFrame calls.
// --device-convert: a .y4m clip's frames are not converted to BGR on the host: the raw planes of a chunk go to vs_stabilizer_process_batch_ycbcr and the
// planes it returns go to the file as they are (the same bytes either way: the device restates video_io.hpp's rule).  For .bgr clips the flag does nothing.
#include <chrono>
#include <filesystem>
#include <iostream>
#include "harness.hpp"

namespace fs = std::filesystem;

// --out-size: w == 0: off (the crop window is written); w == -1: the source frame's size; filter -1: chosen from the sizes
struct OutSize { int w = 0, h = 0, filter = -1; };

// the planes of frame 0 of a chunk of raw y4m frames at `base`, frames back to back in the file's layout (Y, then Cb, then Cr)
static vs_ycbcr_planes planes_of(const vsio::Format& f, void* base) {
    const size_t esz = f.sample_bytes();
    vs_ycbcr_planes p{};
    p.y = base; p.y_stride = f.w; p.c_step = 1;
    p.y_frame_stride = p.c_frame_stride = f.frame_samples();
    if (f.chroma == vsio::Chroma::Mono) return p;
    p.cb = (char*)base + (size_t)f.w * f.h * esz;
    p.cr = (char*)p.cb + (size_t)f.cw() * f.ch() * esz;
    p.c_stride = f.cw();
    p.sub_x = f.chroma == vsio::Chroma::C444 ? 0 : 1; p.sub_y = f.chroma == vsio::Chroma::C420 ? 1 : 0;
    return p;
}

static bool process_clip(const std::string& in_path, const std::string& out_path, vs_stabilizer_params params, int device, int chunk,
                         bool force444, int fill, vs_fill_blend_params blend, int deblur, int denoise, int denoise_strength, int deflicker,
                         int deflicker_step, int scene_cut, int sharpen, bool inpaint, double rolling, const std::vector<double>& lens, double lens_zoom, bool device_convert, OutSize out_size) {
    vsio::Reader reader;
    if (!reader.open(in_path)) { std::cerr << "Error: " << reader.error << std::endl; return false; }
    const vsio::Format fin = reader.fmt;
    const int crop = params.crop_pixels > 0 ? params.crop_pixels : 0;
    vsio::Format fout = fin;
    fout.w = fin.w - 2 * crop; fout.h = fin.h - 2 * crop;             // video_test.cpp:74-76
    if (force444 || fin.chroma == vsio::Chroma::Mono) fout.chroma = vsio::Chroma::C444;
    if (fout.w <= 0 || fout.h <= 0) { std::cerr << "Error: crop larger than the frame" << std::endl; return false; }
    if (out_size.w != 0) {                                              // the writer takes the delivered size (vs_stabilizer_set_output_size)
        const int win_w = fout.w, win_h = fout.h;
        fout.w = out_size.w < 0 ? fin.w : out_size.w; fout.h = out_size.h < 0 ? fin.h : out_size.h;
        // the default filter: area where an axis shrinks by more than 2:1 (and area can take both axes there), linear otherwise
        if (out_size.filter < 0)
            out_size.filter = (win_w > 2 * fout.w || win_h > 2 * fout.h) && fout.w <= win_w && win_w <= 8 * fout.w && fout.h <= win_h && win_h <= 8 * fout.h
                                  ? VS_RESIZE_AREA : VS_RESIZE_LINEAR;
    }
    vsio::Writer writer;
    if (!writer.open(out_path, fout)) { std::cerr << "Error: " << writer.error << std::endl; return false; }
    std::cout << "Input FPS: " << (double)fin.fps_num / fin.fps_den << " | Frame Size: " << fout.w << "x" << fout.h << std::endl;
    std::cout << "Writing processed video to: " << out_path << std::endl;

    const size_t esz = fin.bits > 8 ? 2 : 1;
    const bool planes = device_convert && vsio::ends_with(in_path, ".y4m");      // raw planes in and out, converted on the device
    const size_t in_elems = planes ? fin.frame_samples() : fin.bgr_elems(), out_elems = planes ? fout.frame_samples() : fout.bgr_elems();
    std::vector<uint8_t> h_in((size_t)chunk * in_elems * esz), h_out((size_t)chunk * out_elems * esz);
    vsh::DeviceBuffer d_in(h_in.size()), d_out(h_out.size());
    std::vector<int32_t> has_output((size_t)chunk);
    vs_stabilizer* stab = vs_stabilizer_create(&params, device);
    if (!stab) { std::cerr << "Error: vs_stabilizer_create: " << vs_last_error() << std::endl; return false; }
    if (fill != 0 && vs_stabilizer_set_border_fill(stab, fill) != VS_OK) {
        std::cerr << "Error: vs_stabilizer_set_border_fill: " << vs_last_error() << std::endl;
        vs_stabilizer_destroy(stab);
        return false;
    }
    if ((blend.feather != 0 || blend.match != 0) && vs_stabilizer_set_fill_blend(stab, &blend) != VS_OK) {
        std::cerr << "Error: vs_stabilizer_set_fill_blend: " << vs_last_error() << std::endl;
        vs_stabilizer_destroy(stab);
        return false;
    }
    if (inpaint && vs_stabilizer_set_inpaint(stab, 1) != VS_OK) {
        std::cerr << "Error: vs_stabilizer_set_inpaint: " << vs_last_error() << std::endl;
        vs_stabilizer_destroy(stab);
        return false;
    }
    if (deblur != 0 && vs_stabilizer_set_deblur(stab, deblur, nullptr) != VS_OK) {
        std::cerr << "Error: vs_stabilizer_set_deblur: " << vs_last_error() << std::endl;
        vs_stabilizer_destroy(stab);
        return false;
    }
    if (denoise != 0) {
        vs_denoise_params dp;
        vs_denoise_params_default(&dp);
        if (denoise_strength != 0) dp.strength = denoise_strength;
        if (vs_stabilizer_set_denoise(stab, denoise, &dp) != VS_OK) {
            std::cerr << "Error: vs_stabilizer_set_denoise: " << vs_last_error() << std::endl;
            vs_stabilizer_destroy(stab);
            return false;
        }
    }
    if (deflicker != 0) {
        vs_deflicker_params fp;
        vs_deflicker_params_default(&fp);
        if (deflicker_step != 0) fp.step = deflicker_step;
        if (vs_stabilizer_set_deflicker(stab, deflicker, &fp) != VS_OK) {
            std::cerr << "Error: vs_stabilizer_set_deflicker: " << vs_last_error() << std::endl;
            vs_stabilizer_destroy(stab);
            return false;
        }
    }
    if (scene_cut >= 0) {
        vs_scene_params sp;
        vs_scene_params_default(&sp);
        if (scene_cut != 0) sp.threshold = scene_cut;
        if (vs_stabilizer_set_scene_cut(stab, &sp) != VS_OK) {
            std::cerr << "Error: vs_stabilizer_set_scene_cut: " << vs_last_error() << std::endl;
            vs_stabilizer_destroy(stab);
            return false;
        }
    }
    if (sharpen >= 0) {
        vs_sharpen_params hp;
        vs_sharpen_params_default(&hp);
        if (sharpen != 0) hp.strength = sharpen;
        if (vs_stabilizer_set_sharpen(stab, &hp) != VS_OK) {
            std::cerr << "Error: vs_stabilizer_set_sharpen: " << vs_last_error() << std::endl;
            vs_stabilizer_destroy(stab);
            return false;
        }
    }
    if (out_size.w != 0 && vs_stabilizer_set_output_size(stab, out_size.w, out_size.h, out_size.filter) != VS_OK) {
        std::cerr << "Error: vs_stabilizer_set_output_size: " << vs_last_error() << std::endl;
        vs_stabilizer_destroy(stab);
        return false;
    }
    if (rolling != 0.0) {
        const vs_rolling_params rp{rolling};
        if (vs_stabilizer_set_rolling_shutter(stab, &rp) != VS_OK) {
            std::cerr << "Error: vs_stabilizer_set_rolling_shutter: " << vs_last_error() << std::endl;
            vs_stabilizer_destroy(stab);
            return false;
        }
    }
    if (!lens.empty()) {
        vs_lens_params lp;
        vs_lens_params_default(&lp, fin.w, fin.h);
        double* const field[12] = {&lp.fx, &lp.fy, &lp.cx, &lp.cy, &lp.k1, &lp.k2, &lp.p1, &lp.p2, &lp.k3, &lp.k4, &lp.k5, &lp.k6};
        for (size_t k = 0; k < lens.size(); k++) *field[k] = lens[k];
        lp.zoom = lens_zoom;
        if (vs_stabilizer_set_lens(stab, &lp, fin.w, fin.h) != VS_OK) {
            std::cerr << "Error: vs_stabilizer_set_lens: " << vs_last_error() << std::endl;
            vs_stabilizer_destroy(stab);
            return false;
        }
    }

    long frame_count = 0, written = 0, next_report = 100;
    const auto t0 = std::chrono::steady_clock::now();
    bool ok = true;
    for (;;) {
        int n = 0;
        while (n < chunk && (planes ? reader.next_planes(h_in.data() + (size_t)n * in_elems * esz) : reader.next(h_in.data() + (size_t)n * in_elems * esz))) n++;
        if (n == 0) break;
        if (planes) {
            int ow = 0, oh = 0;
            const vs_ycbcr_planes pin = planes_of(fin, h_in.data()), pout = planes_of(fout, h_out.data());
            const int r = vs_stabilizer_process_batch_ycbcr(stab, &pin, n, fin.w, fin.h, vsh::vs_format_of(fin), VS_MEM_HOST, &pout, has_output.data(), &ow, &oh);
            if (r < 0) { std::cerr << "Error: vs_stabilizer_process_batch_ycbcr: " << vs_last_error() << std::endl; ok = false; break; }
            for (int i = 0; i < n; i++)
                if (has_output[i]) { writer.write_planes(h_out.data() + (size_t)i * out_elems * esz); written++; }
            frame_count += n;
            while (frame_count >= next_report) { std::cout << "Processed " << next_report << " frames..." << std::endl; next_report += 100; }
            if (n < chunk) break;
            continue;
        }
        vsh::hip_check(hipMemcpy(d_in.ptr, h_in.data(), (size_t)n * in_elems * esz, hipMemcpyHostToDevice), "hipMemcpy H2D");
        int ow = 0, oh = 0;
        const int r = vs_stabilizer_process_batch(stab, d_in.ptr, in_elems, n, fin.w, fin.h, fin.w * 3, vsh::vs_format_of(fin), VS_MEM_DEVICE,
                                                  d_out.ptr, out_elems, has_output.data(), &ow, &oh);
        if (r < 0) { std::cerr << "Error: vs_stabilizer_process_batch: " << vs_last_error() << std::endl; ok = false; break; }
        if (r > 0) vsh::hip_check(hipMemcpy(h_out.data(), d_out.ptr, (size_t)n * out_elems * esz, hipMemcpyDeviceToHost), "hipMemcpy D2H");
        for (int i = 0; i < n; i++) {
            // the reference hands the empty Mat of the first `lag` frames to the writer, which drops it (video_test.cpp:104-109)
            if (has_output[i]) { writer.write(h_out.data() + (size_t)i * out_elems * esz); written++; }
        }
        frame_count += n;
        while (frame_count >= next_report) { std::cout << "Processed " << next_report << " frames..." << std::endl; next_report += 100; }
        if (n < chunk) break;
    }
    if (!reader.error.empty()) { std::cerr << "Error: " << reader.error << std::endl; ok = false; }
    if (scene_cut >= 0 && ok) {                                         // the clip's cut list (the most recent 256)
        int64_t cuts[256];
        const int total = vs_stabilizer_get_scene_cuts(stab, cuts, 256);
        std::cout << "Scene cuts: " << total << " [";
        for (int k = 0; k < std::min(total, 256); k++) std::cout << (k ? ", " : "") << cuts[k];
        std::cout << "]" << std::endl;
    }
    vs_stabilizer_destroy(stab);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::cout << "Finished processing " << frame_count << " frames (" << written << " written, " << frame_count / std::max(sec, 1e-9)
              << " frames/s incl. file I/O) for video: " << fs::path(in_path).filename().string() << std::endl;
    return ok;
}

int main(int argc, char** argv) {
    std::string input_dir = "../recordings", output_dir = "output";   // video_test.cpp:12-13
    int chunk = 64, device = 0, crop = 0, fill = 0, deblur = 0, denoise = 0, denoise_strength = 0, deflicker = 0, deflicker_step = 0, scene_cut = -1, sharpen = -1, positional = 0;
    bool bilinear = false, lanczos2 = false, force444 = false, device_convert = false;
    vs_fill_blend_params blend{0, 0};
    bool inpaint = false;
    double rolling = 0.0, lens_zoom = 1.0;
    std::vector<double> lens;                              // --lens: 8, 9 or 12 numbers
    OutSize out_size;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--chunk" && i + 1 < argc) chunk = std::max(1, std::atoi(argv[++i]));
        else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--crop" && i + 1 < argc) crop = std::atoi(argv[++i]);
        else if (a == "--fill" && i + 1 < argc) fill = std::atoi(argv[++i]);
        else if (a == "--fill-feather" && i + 1 < argc) blend.feather = std::atoi(argv[++i]);
        else if (a == "--fill-match") blend.match = 1;
        else if (a == "--inpaint") inpaint = true;
        else if (a == "--deblur" && i + 1 < argc) deblur = std::atoi(argv[++i]);
        else if (a == "--denoise" && i + 1 < argc) denoise = std::atoi(argv[++i]);
        else if (a == "--denoise-strength" && i + 1 < argc) denoise_strength = std::atoi(argv[++i]);
        else if (a == "--deflicker" && i + 1 < argc) deflicker = std::atoi(argv[++i]);
        else if (a == "--deflicker-step" && i + 1 < argc) deflicker_step = std::atoi(argv[++i]);
        else if (a == "--scene-cut") {                          // (-1: off, 0: the default threshold)
            scene_cut = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' && std::string(argv[i + 1]).find_first_not_of("0123456789") == std::string::npos) {
                scene_cut = std::atoi(argv[++i]);
                if (scene_cut == 0) scene_cut = 256;           // (0 is not a threshold: refused by the library like any value outside 1 .. 255)
            }
        }
        else if (a == "--sharpen") {                            // (-1: off, 0: the default strength)
            sharpen = 0;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' && std::string(argv[i + 1]).find_first_not_of("0123456789") == std::string::npos) {
                sharpen = std::atoi(argv[++i]);
                if (sharpen == 0) sharpen = 33;                // (0 is not a strength: refused by the library like any value outside 1 .. 32)
            }
        }
        else if (a == "--rolling-shutter" && i + 1 < argc) rolling = std::atof(argv[++i]);
        else if (a == "--lens" && i + 1 < argc) {
            lens.clear();
            for (const char* p = argv[++i]; *p;) {
                char* e;
                lens.push_back(std::strtod(p, &e));
                if (e == p) { lens.clear(); break; }
                p = *e == ',' ? e + 1 : e;
                if (*e && *e != ',') { lens.clear(); break; }
            }
            if (lens.size() != 8 && lens.size() != 9 && lens.size() != 12) { std::cerr << "Error: --lens takes fx,fy,cx,cy,k1,k2,p1,p2[,k3[,k4,k5,k6]]\n"; return EXIT_FAILURE; }
        }
        else if (a == "--lens-zoom" && i + 1 < argc) lens_zoom = std::atof(argv[++i]);
        else if (a == "--bilinear") bilinear = true;
        else if (a == "--lanczos2") lanczos2 = true;
        else if (a == "--444") force444 = true;
        else if (a == "--device-convert") device_convert = true;
        else if (a == "--out-size" && i + 1 < argc) {
            const std::string v = argv[++i];
            char x = 0;
            if (v == "source") out_size.w = out_size.h = -1;
            else if (std::sscanf(v.c_str(), "%d%c%d", &out_size.w, &x, &out_size.h) != 3 || x != 'x' || out_size.w < 1 || out_size.h < 1) {
                std::cerr << "Error: --out-size takes WxH or source\n"; return EXIT_FAILURE;
            }
        }
        else if (a == "--out-filter" && i + 1 < argc) {
            const std::string v = argv[++i];
            if (v == "linear") out_size.filter = VS_RESIZE_LINEAR;
            else if (v == "area") out_size.filter = VS_RESIZE_AREA;
            else { std::cerr << "Error: --out-filter takes linear or area\n"; return EXIT_FAILURE; }
        }
        else if (positional == 0) { input_dir = a; positional++; }
        else if (positional == 1) { output_dir = a; positional++; }
        else { std::cerr << "Usage: " << argv[0] << " [input_dir] [output_dir] [--chunk N] [--device D] [--crop N] [--fill N] [--fill-feather N] [--fill-match] [--inpaint] [--deblur N] [--denoise N] [--denoise-strength T] [--deflicker N] [--deflicker-step S] [--scene-cut [T]] [--sharpen [S]] [--rolling-shutter R] [--lens fx,fy,cx,cy,k1,k2,p1,p2[,k3[,k4,k5,k6]]] [--lens-zoom Z] [--bilinear] [--444] [--device-convert] [--out-size WxH | source] [--out-filter linear|area]\n"; return EXIT_FAILURE; }
    }
    try {
        if (!fs::exists(output_dir)) {
            fs::create_directories(output_dir);
            std::cout << "Created output directory: " << output_dir << std::endl;
        }
        if (!fs::is_directory(input_dir)) { std::cerr << "Error: Input directory does not exist or is not a directory.\n"; return EXIT_FAILURE; }
        std::vector<std::string> clips;
        for (const auto& e : fs::directory_iterator(input_dir)) {
            const std::string ext = e.path().extension().string();
            if (e.is_regular_file() && (ext == ".y4m" || ext == ".bgr")) clips.push_back(e.path().filename().string());
        }
        std::sort(clips.begin(), clips.end());
        if (clips.empty()) { std::cerr << "No .y4m / .bgr clips found in the input directory: " << input_dir << std::endl; return EXIT_FAILURE; }
        if (vs_device_count() <= device) { std::cerr << "Error: no HIP device " << device << std::endl; return EXIT_FAILURE; }

        vs_stabilizer_params params;
        vs_stabilizer_params_default(&params);
        params.crop_pixels = crop;                         // 0: disable crop so we can see what it is doing (video_test.cpp:55)
        if (bilinear) params.warp_mode = VS_WARP_BILINEAR;    // the Halide sampler's float lerp (the default is cv::warpAffine's fixed-point bilinear, VS_WARP_BILINEAR_CV)
        if (lanczos2) params.warp_mode = VS_WARP_LANCZOS2;
        int failed = 0;
        for (const auto& name : clips) {
            const std::string in_path = (fs::path(input_dir) / name).string();
            std::cout << "\nProcessing video: " << in_path << std::endl;
            if (!process_clip(in_path, (fs::path(output_dir) / ("processed_" + name)).string(), params, device, chunk, force444, fill, blend, deblur, denoise, denoise_strength, deflicker, deflicker_step, scene_cut, sharpen, inpaint, rolling, lens, lens_zoom, device_convert, out_size)) failed++;
        }
        if (failed) { std::cerr << "\n" << failed << " clip(s) failed." << std::endl; return EXIT_FAILURE; }
        std::cout << "\nAll videos have been processed successfully." << std::endl;
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}
