// vs_eval_fidelity -- picture scores of clips from the library's fidelity statistics (fidelity.hpp; include/vs_amd.h, THE FIDELITY RULE).
//   vs_eval_fidelity [--device D] [--frames M] [--inset C] [--chunk K] [--ref clip] clip1 [clip2 ...]
// Without --ref, per clip:  "<path>\titf_psnr_db=<v>\titf_psnr_y_db=<v>\titf_ssim=<v>" -- the means over consecutive frame pairs of min(psnr, 100),
// min(psnr_y, 100) and ssim.  With --ref, frame i of the clip against frame i of the reference:  "<path>\tpsnr_db=<v>\tpsnr_y_db=<v>\tssim=<v>",
// averaged the same way; a reference of another size or depth is an error.  The image is the frame minus C pixels on every side (--inset: a
// stabilized clip's border shows whatever the warp's border mode put there).  --chunk: frames per upload (default: about 256 MiB).
#include <iostream>
#include "fidelity.hpp"

int main(int argc, char** argv) {
    int device = 0, inset = 0;
    size_t max_frames = 0, chunk = 0;
    std::string ref_path;
    std::vector<std::string> paths;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--frames" && i + 1 < argc) max_frames = (size_t)std::max(0, std::atoi(argv[++i]));
        else if (a == "--inset" && i + 1 < argc) inset = std::atoi(argv[++i]);
        else if (a == "--chunk" && i + 1 < argc) chunk = (size_t)std::max(0, std::atoi(argv[++i]));
        else if (a == "--ref" && i + 1 < argc) ref_path = argv[++i];
        else paths.push_back(a);
    }
    if (paths.empty() || inset < 0) {
        std::cerr << "Usage: " << argv[0] << " [--device D] [--frames M] [--inset C] [--chunk K] [--ref clip] video1 [video2 ...]\n";
        return 1;
    }
    int rc = 0;
    try {
        if (vs_device_count() < 1) { std::cerr << "No HIP device: the fidelity statistics run on the GPU only\n"; return 1; }
        vsh::hip_check(hipSetDevice(device), "hipSetDevice");
        const bool with_ref = !ref_path.empty();
        vsio::Clip ref;
        std::string err;
        if (with_ref && !vsio::load_clip(ref_path, ref, err, max_frames)) { std::cerr << "Cannot open reference: " << ref_path << " (" << err << ")\n"; return 1; }
        std::cerr << vsfid::score_note(with_ref) << std::endl;
        for (const auto& path : paths) {
            vsio::Clip clip;
            if (!vsio::load_clip(path, clip, err, max_frames)) { std::cerr << "Cannot open video: " << path << " (" << err << ")\n"; continue; }
            if (clip.frames < (with_ref ? 1u : 2u)) { std::cerr << "Too few frames: " << path << "\n"; continue; }
            try {
                const vsfid::Means m = vsfid::measure(clip, with_ref ? &ref : nullptr, inset, chunk);
                const char* const pre = with_ref ? "" : "itf_";
                std::cout << path << "\t" << pre << "psnr_db=" << m.mean_psnr() << "\t" << pre << "psnr_y_db=" << m.mean_psnr_y() << "\t" << pre << "ssim=" << m.mean_ssim()
                          << "\n";
            } catch (const std::exception& e) {
                std::cerr << "Error: " << path << ": " << e.what() << "\n";
                rc = 1;
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "Error: " << e.what() << "\n";
        return 1;
    }
    return rc;
}
