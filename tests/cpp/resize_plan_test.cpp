// What a stabilizer call delivers (video_stabilizer_amd/csrc/vs_stab_plan.hpp: PassConfig's output size, delivered_size) against values worked
// out by hand.  Host only: built with the address and undefined-behaviour sanitizers together with csrc/vs_host.cpp
// (tests/test_resize_plan_cpp.py).
#include "../../video_stabilizer_amd/csrc/vs_stab_plan.hpp"

#include <cstdio>

using namespace vsi::stab;

static int failures = 0;
static void expect(bool cond, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (!cond) { if (failures < 40) printf("FAIL %s (%lld %lld %lld)\n", what, a, b, c); failures++; }
}
static bool is(const Delivery& d, int w, int h, bool resize) { return d.w == w && d.h == h && d.resize == resize; }

int main() {
    PassConfig c;
    expect(c.out_w == 0 && c.out_h == 0 && c.out_filter == VS_RESIZE_LINEAR, "off by default, the linear filter");
    // off: the crop window, whatever the crop
    expect(is(delivered_size(1920, 1080, 32, c), 1856, 1016, false), "off: 1080p at crop 32 leaves as 1856 x 1016");
    expect(is(delivered_size(1920, 1080, 0, c), 1920, 1080, false), "off: crop 0");
    expect(is(delivered_size(160, 128, 8, c), 144, 112, false), "off: 160 x 128 at crop 8");
    // the source frame's size: a resize unless the crop is 0
    c.out_w = c.out_h = -1;
    expect(is(delivered_size(1920, 1080, 32, c), 1920, 1080, true), "source: zoom to fill");
    expect(is(delivered_size(1920, 1080, 0, c), 1920, 1080, false), "source at crop 0: the window has that size already");
    expect(is(delivered_size(3840, 2160, 64, c), 3840, 2160, true), "source: 4K at crop 64");
    // a fixed size: a resize unless the window has it
    c.out_w = 1920; c.out_h = 1080;
    expect(is(delivered_size(3840, 2160, 32, c), 1920, 1080, true), "a 4K master leaves as a 1080p proxy");
    expect(is(delivered_size(1984, 1144, 32, c), 1920, 1080, false), "the window is 1920 x 1080 already");
    expect(is(delivered_size(1984, 1080, 32, c), 1920, 1080, true), "one axis differs");
    expect(is(delivered_size(1920, 1144, 32, c), 1920, 1080, true), "the other axis differs");
    c.out_w = 144; c.out_h = 112; c.out_filter = VS_RESIZE_AREA;
    expect(is(delivered_size(160, 128, 8, c), 144, 112, false), "the filter does not make a resize of an equal size");
    expect(is(delivered_size(160, 128, 0, c), 144, 112, true), "the same size from a larger window");
    if (!failures) printf("ALL PASS\n");
    return failures ? 1 : 0;
}
