// vs_launch.hpp -- the host side that the kernel launchers share: which containers a pass takes, the walk over a call's frames in launches
// the grid allows, and the test that lets a lane own four pixels.  Plain C++ with no HIP types: tests/cpp/launch_shape_test.cpp compiles it
// alone.
#pragma once

#include <cstddef>
#include <cstdint>

namespace vsk {

// the containers the fixed-point passes take: 8 bits with every value in use, 16 bits with the format's maximum
inline bool container_ok(int bits, int max_value) {
    return !(bits == 16 ? (max_value < 0 || max_value > 65535) : (bits != 8 || max_value != 255));
}

// f(first, count) over [0, n) in order, count <= 65535: a launch takes that many frames (or frame groups) at the most
constexpr int kMaxFramesPerLaunch = 65535;                 // gridDim.y limit
template <typename F>
inline void for_frame_chunks(int n, F&& f) {
    for (int f0 = 0; f0 < n; f0 += kMaxFramesPerLaunch) f(f0, n - f0 < kMaxFramesPerLaunch ? n - f0 : kMaxFramesPerLaunch);
}

// every row of every frame of one surface starts on a dword: dword accesses, so four 8-bit pixels (or two 16-bit ones) per lane.  p: the first
// frame (null: only the strides are asked about); stride, frame_stride: in elements of esz bytes; frame_stride counts where n_frames > 1.
// A launcher asks this of each surface it reads or writes as dwords, and of nothing else.
inline bool rows_on_dwords(const void* p, size_t stride, size_t frame_stride, int n_frames, size_t esz) {
    return (((uintptr_t)p | (stride * esz) | (n_frames > 1 ? frame_stride * esz : 0)) & 3) == 0;
}

}  // namespace vsk
