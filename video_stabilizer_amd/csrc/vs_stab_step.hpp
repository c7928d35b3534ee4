// vs_stab_step.hpp -- the scalar bookkeeping of one VideoStabilizer::processFrame (stabilizer.cpp:35-99).  Host only, no HIP.
#pragma once

#include "../../include/vs_amd.h"

#include <algorithm>
#include <deque>

namespace vsi {

// The earliest queued measurement is finalised (stabilizer.cpp:56-99): its jitter (against the smoothed path, or the measurement itself with the
// smoother off) joins `accum`, which decays by how far it moves the frame's corners; *correction = inverse(the new accum).
inline void stab_finalise(const vs_transform& earliest, const vs_transform& earliest_smoothed, int w, int h, const vs_stabilizer_params& p, vs_transform& accum,
                          vs_transform* correction) {
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
}

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
    stab_finalise(earliest, earliest_smoothed, w, h, p, accum, correction);
    return true;
}

// stab_step with scene cuts (the rule: vs_scene.hip).  `cut`: this frame shows another scene than the frame before it;
// `cuts` runs beside `measurements` and `ok`, entry for entry.  With cut == false on every frame this is stab_step, bit for bit
// (tests/cpp/scene_step_test.cpp).  A cut frame
//   - enters the smoother and the queue with the identity as its measurement: what the aligner made of two unrelated images is no motion;
//   - is queued with ok == 0, so every candidate list ends in front of it (vs_lookahead.hpp);
//   - leaves `accum` alone on arrival -- the reference's arrival-time reset stays for failed alignments only: the `lag` frames of the old scene
//     that are still queued would jerk;
//   - when it is itself finalised, has the identity as its jitter and makes `accum` the identity: *correction is inverse(identity), and the new
//     scene starts from a clean path.
// A frame that is both failed and cut gets both treatments.
inline bool stab_step_cut(const vs_transform& meas, bool success, bool cut, int w, int h, const vs_stabilizer_params& p, vs_smoother* smoother,
                          std::deque<vs_transform>& measurements, std::deque<int>& ok, std::deque<int>& cuts, vs_transform& accum, vs_transform* correction) {
    const vs_transform m = cut ? vs_transform{0, 0, 0, 0} : meas;
    vs_transform earliest_smoothed{0, 0, 0, 0};
    if (p.enable_smoother) (void)vs_smoother_update(smoother, &m, &earliest_smoothed);
    if (!success) accum = vs_transform{0, 0, 0, 0};
    measurements.push_back(m);
    ok.push_back(success && !cut ? 1 : 0);
    cuts.push_back(cut ? 1 : 0);
    if (measurements.size() <= (size_t)p.lag) return false;
    vs_transform earliest = measurements.front();
    const bool earliest_cut = cuts.front() != 0;
    measurements.pop_front();
    ok.pop_front();
    cuts.pop_front();
    if (earliest_cut) {
        accum = vs_transform{0, 0, 0, 0};
        *correction = vs_transform_inverse(&accum);
        return true;
    }
    stab_finalise(earliest, earliest_smoothed, w, h, p, accum, correction);
    return true;
}

}  // namespace vsi
