// vs_lens.hpp -- the radial lens map's rule (include/vs_amd.h: vs_lens_map), written once for the host (vs_host.cpp: vsi::lens_map_host) and
// the device (vs_remap.hip: vs_k_lens_map).  Only + - * / and rint, every operation rounds once in the order written (every file that
// includes this one is compiled with -ffp-contract=off), so both sides and the numpy restatement (tests/_lens_ref.py) give the same bits.
// Plain C++: tests/cpp/lens_map_test.cpp builds it with g++.
#pragma once

#include "../../include/vs_amd.h"

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VS_LENS_HD __host__ __device__ __forceinline__
#else
#define VS_LENS_HD inline
#endif

namespace vsl {

// cvRound with saturation: ties to even, NaN -> 0 (vs_device.hpp: cv_round_sat, operation for operation; 2147483647.0 is exact in fp64, so the
// conversion is of an integer inside the int range)
VS_LENS_HD int round_sat(double v) {
    if (!(v == v)) return 0;
    return (int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0);
}

// what vs_lens_map and vs_stabilizer_set_lens accept: every parameter finite, fx, fy and zoom > 0
VS_LENS_HD bool params_ok(const vs_lens_params& p) {
    const double v[13] = {p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.p1, p.p2, p.k3, p.k4, p.k5, p.k6, p.zoom};
    for (int i = 0; i < 13; i++)
        if (!(v[i] - v[i] == 0.0)) return false;                       // (an infinity or a NaN minus itself is NaN)
    return p.fx > 0.0 && p.fy > 0.0 && p.zoom > 0.0;
}
// all eight coefficients 0 and zoom 1: the map is (32 u, 32 v)
VS_LENS_HD bool is_identity(const vs_lens_params& p) {
    return p.k1 == 0.0 && p.k2 == 0.0 && p.p1 == 0.0 && p.p2 == 0.0 && p.k3 == 0.0 && p.k4 == 0.0 && p.k5 == 0.0 && p.k6 == 0.0 && p.zoom == 1.0;
}

// THE RULE: where output pixel (u, v) lies in the distorted frame, 5 fraction bits
VS_LENS_HD void position(const vs_lens_params& p, int u, int v, int32_t* X, int32_t* Y) {
    const double x = ((double)u - p.cx) / (p.fx * p.zoom), y = ((double)v - p.cy) / (p.fy * p.zoom);
    const double r2 = x * x + y * y;
    const double kr = (1.0 + ((p.k3 * r2 + p.k2) * r2 + p.k1) * r2) / (1.0 + ((p.k6 * r2 + p.k5) * r2 + p.k4) * r2);
    const double xy2 = 2.0 * (x * y);
    const double xd = x * kr + (p.p1 * xy2 + p.p2 * (r2 + 2.0 * (x * x)));
    const double yd = y * kr + (p.p1 * (r2 + 2.0 * (y * y)) + p.p2 * xy2);
    *X = round_sat((p.fx * xd + p.cx) * 32.0);
    *Y = round_sat((p.fy * yd + p.cy) * 32.0);
}

}  // namespace vsl
