// vs_stab_step.hpp -- the scalar bookkeeping of one VideoStabilizer::processFrame (stabilizer.cpp:35-99).  Host only, no HIP.
#pragma once

#include "../../include/vs_amd.h"

#include <algorithm>
#include <deque>

namespace vsi {

// One frame's measurement enters: the smoother takes it, a failed alignment resets the accumulated correction, the measurement is queued; once
// more than `lag` are queued the earliest one is finalised -- its jitter (against the smoothed path, or the measurement itself with the smoother
// off) joins `accum`, which decays by how far it moves the frame's corners.  Returns whether a measurement was finalised; then *correction =
// inverse(the new accum), what the reference hands to its warp (:97-99).  `ok` runs beside `measurements`, entry for entry (vs_lookahead.hpp
// reads both).  The arithmetic is these calls in this order -- the translation units are built with -ffp-contract=off, so every caller gets the
// same bits (tests/cpp/stab_step_test.cpp: against the oracle's step).
inline bool stab_step(const vs_transform& meas, bool success, int w, int h, const vs_stabilizer_params& p, vs_smoother* smoother,
                      std::deque<vs_transform>& measurements, std::deque<int>& ok, vs_transform& accum, vs_transform* correction) {
    vs_transform earliest_smoothed{0, 0, 0, 0};
    if (p.enable_smoother) (void)vs_smoother_update(smoother, &meas, &earliest_smoothed);   // :35
    if (!success) accum = vs_transform{0, 0, 0, 0};                                         // :39-41
    measurements.push_back(meas);                                                           // :44
    ok.push_back(success ? 1 : 0);
    if (measurements.size() <= (size_t)p.lag) return false;                                 // :48
    vs_transform earliest = measurements.front();
    measurements.pop_front();
    ok.pop_front();
    vs_transform jitter;
    if (p.enable_smoother) {
        vs_transform inv = vs_transform_inverse(&earliest_smoothed);
        jitter = vs_transform_compose(&earliest, &inv);                                     // :60
    } else {
        jitter = earliest;
    }
    vs_transform na = vs_transform_compose(&accum, &jitter);                                // :66
    const double disp = vs_transform_max_corner_displacement(&na, w, h);                    // :69-70
    double decay;
    if (disp > p.max_disp) {
        decay = p.max_decay;
    } else if (disp > p.min_disp) {
        double f = (disp - p.min_disp) / (p.max_disp - p.min_disp);
        f = std::max(0.0, std::min(1.0, f));
        decay = p.min_decay * (1.0 - f) + p.max_decay * f;
    } else {
        decay = p.min_decay;
    }
    na.TX *= decay; na.TY *= decay; na.A *= decay; na.B *= decay;                           // :88-91
    accum = na;
    *correction = vs_transform_inverse(&na);
    return true;
}

}  // namespace vsi
