// vs_lookahead.hpp -- the candidate transforms of the stabilizer's look-ahead passes (border fill, deblur, denoise, deflicker).  Host only, no HIP.
#pragma once

#include "../../include/vs_amd.h"

#include <stddef.h>

namespace vsi {

// Frame k leaves the queue; the queue now holds the frames k+1 .. behind it and meas[c] is the motion T_{k+1+c} (T_j: frame j-1 to j), entry
// for entry, with ok[c] its alignment's success.  Frame k+1+c shows frame k's pixels through inverse(T_{k+1} o .. o T_{k+1+c}); with a
// `correction` (the fill: what frame k itself is warped by) it shows the OUTPUT through compose(that, correction).  The list ends at the first
// of: n_ahead entries, `avail` queued frames, a failed alignment.  out[0 .. n_ahead): the live entries, then {0, 0, 0, 0}.  Returns the live count.
// Meas / Ok: anything indexable (the engine's deques, arrays).  The arithmetic is these calls in this order -- the translation units are built
// with -ffp-contract=off, so every caller gets the same bits.
template <typename Meas, typename Ok>
inline int lookahead_transforms(const Meas& meas, const Ok& ok, size_t avail, int n_ahead, const vs_transform* correction, vs_transform* out) {
    vs_transform chain{0, 0, 0, 0};
    int live = 0;
    for (; live < n_ahead && (size_t)live < avail && ok[live]; live++) {
        chain = vs_transform_compose(&chain, &meas[live]);
        const vs_transform back = vs_transform_inverse(&chain);
        out[live] = correction ? vs_transform_compose(&back, correction) : back;
    }
    for (int c = live; c < n_ahead; c++) out[c] = vs_transform{0, 0, 0, 0};
    return live;
}

}  // namespace vsi
