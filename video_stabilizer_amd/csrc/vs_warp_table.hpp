// vs_warp_table.hpp -- the layout of the per-launch tables of the float-tile Lanczos2 warp (vs_warp.hip: vs_k_warp_c3_tables writes them, the
// contracted and separable forms of vs_k_bgr_warp_c3 read them with scalar loads).  Per frame, back to back:
//   tiles  16-byte entries {int sx_lo, int sy_lo, rows | groups << 16, fits | interior << 1}, one per 64 x 16 output tile in raster order;
//   rows   8-byte pairs {fl(B * fy), fl(A1 * fy)}, one per output row, the run rounded up to whole 4-row blocks (rows beyond the window repeat
//          its last row), so that the four rows a wave samples in one block are one aligned 32-byte scalar load.
// Plain C++: the sizing is tested on the host (tests/test_warp_table_cpp.py).
#pragma once

#include <cstddef>

namespace vsk {

constexpr int kWarpTabTileW = 64, kWarpTabTileH = 16, kWarpTabRowBlock = 4;

struct WarpTableLayout { size_t tiles, rows, bytes; };      // per frame; bytes is a multiple of 16

inline WarpTableLayout warp_c3_table_layout(int roi_w, int roi_h) {
    if (roi_w < 1 || roi_h < 1) return WarpTableLayout{0, 0, 0};
    const size_t tx = ((size_t)roi_w + kWarpTabTileW - 1) / kWarpTabTileW, ty = ((size_t)roi_h + kWarpTabTileH - 1) / kWarpTabTileH;
    const size_t rows = ((size_t)roi_h + kWarpTabRowBlock - 1) / kWarpTabRowBlock * kWarpTabRowBlock;
    return WarpTableLayout{tx * ty, rows, 16 * tx * ty + 8 * rows};
}

}  // namespace vsk
