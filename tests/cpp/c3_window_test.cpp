// The tile-window decision of the float-tile warps (video_stabilizer_amd/csrc/vs_c3_window.hpp: vsd::c3_tile_window, c3_extents,
// c3_compact_shape) against the sampler's own positions, pixel by pixel.  Two uses (tests/test_c3_window_cpp.py drives both):
//
//   c3_window_test grid     walks a built-in grid of maps x shifts x windows x instantiations x {extents, four corners} and asks of every tile
//       SOUND    fits => every live pixel's tap window (4 x 4 from floor - 1 on the float tiles, 2 x 2 from floor on the raw tiles) lies in
//                [sx_lo, sx_lo + 4 groups) x [sy_lo, sy_lo + rows), positions formed as the sampler forms them, in the plain and in the tabled
//                order of operations
//       EXACT    fits => the sampler's fp32 offset expression (vs_warp.hip, place(), restated below) equals the integer offset, for every pixel
//       REFUSED  fits => 1 <= rows <= max_rows, 1 <= groups <= max_groups; a footprint at 10^6 or beyond never fits
//       COMPACT  c3_compact_shape admits a frame to shape 1 / 2 only when every tile's footprint is within 20 rows / 18 groups
//     of the function, and the first three of THE FORM IT REPLACED (kept below for that alone), per instantiation: one line each
//       "<shape> tiles T fits F | new unsound U inexact X oversized O | old fits F unsound U inexact X far_row_cases C far_row_inexact I"
//     then "COMPACT checked N bad B" and "DONE".  Violations of the new form are printed ("BAD ...", the first twenty).
//
//   c3_window_test cases    a filter: every line of stdin is "A B TX TY w h rx ry rw rh shape with_extents" -- the transform's four doubles as
//     hex floats, the frame, the window, the instantiation's index in kShapes, 0 / 1.  The parameters are made as the C ABI makes them
//     (vs_ul_params_warp), the extents by c3_extents; out come "E <four hex floats> <compact shape>", one line "x0 y0 fits sx_lo sy_lo rows
//     groups" per tile in raster order and "END <tiles>".
//
// Host only: built with -ffp-contract=off and the address and undefined-behaviour sanitizers together with csrc/vs_host.cpp.
#include "../../video_stabilizer_amd/csrc/vs_c3_window.hpp"
#include "../../include/vs_amd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int kTileW = 64;
struct Shape { const char* name; int tile_h; vsd::C3Staged st; int scale; bool tabled; };
// every instantiation of vs_k_bgr_warp_c3: {tile height, {staged rows, column groups, pitch, org}, bytes per staged pixel}
const Shape kShapes[] = {
    {"standard_24x20x81", 16, {24, 20, 81, 1}, 16, true},  {"six_wave_20x20x81", 16, {20, 20, 81, 1}, 16, true},
    {"seven_wave_20x18x73", 16, {20, 18, 73, 1}, 16, true}, {"raw_u8_40x20x88", 32, {40, 20, 88, 0}, 4, false},
    {"raw_u16_24x20x88", 16, {24, 20, 88, 0}, 8, false},
};
constexpr int kNShapes = (int)(sizeof kShapes / sizeof kShapes[0]);

// THE FORM THIS REPLACED (vs_warp.hip's geom() and vs_k_warp_c3_tables until the decision moved into vs_c3_window.hpp), kept here only to show
// that the grid reaches its fault: the same footprint, "fits" by the magnitudes and the window's extent alone.
vsd::C3Window replaced_form(vsd::C3Tile t, vsd::C3Roi roi, vsd::C3Params p, bool with_extents, vsd::C3Extents E, vsd::C3Staged s) {
    const float A1 = p.A1, B = p.B, TX = p.TX, TY = p.TY;
    const int x0 = t.x0, y0 = t.y0;
    const int x1 = std::min(x0 + t.tile_w, roi.w) - 1, y1 = std::min(y0 + t.tile_h, roi.h) - 1;
    const float fx0 = (float)(x0 + roi.x), fx1 = (float)(x1 + roi.x), fy0 = (float)(y0 + roi.y), fy1 = (float)(y1 + roi.y);
    float mnx, mxx, mny, mxy;
    if (with_extents) {
        const float Wx00 = A1 * fx0 - B * fy0 + TX, Wy00 = B * fx0 + A1 * fy0 + TY;
        mnx = Wx00 + E.lo_x; mxx = Wx00 + E.hi_x; mny = Wy00 + E.lo_y; mxy = Wy00 + E.hi_y;
    } else {
        const float xa = A1 >= 0.f ? fx0 : fx1, xb = A1 >= 0.f ? fx1 : fx0;
        const float ya = B >= 0.f ? fy0 : fy1, yb = B >= 0.f ? fy1 : fy0;
        mnx = A1 * xa - B * yb + TX; mxx = A1 * xb - B * ya + TX;
        const float xc = B >= 0.f ? fx0 : fx1, xd = B >= 0.f ? fx1 : fx0;
        const float yc = A1 >= 0.f ? fy0 : fy1, yd = A1 >= 0.f ? fy1 : fy0;
        mny = B * xc + A1 * yc + TY; mxy = B * xd + A1 * yd + TY;
    }
    bool fits = fmaxf(fmaxf(fabsf(mnx), fabsf(mxx)), fmaxf(fabsf(mny), fabsf(mxy))) < 1.0e6f;
    int sx_lo = 0, sy_lo = 0, rows = 0, groups = 0;
    if (fits) {
        sx_lo = ((int)floorf(mnx) - 1) & ~3;
        const int sx_hi = (int)floorf(mxx) + 2;
        sy_lo = (int)floorf(mny) - 1;
        const int sy_hi = (int)floorf(mxy) + 2;
        rows = sy_hi - sy_lo + 1;
        groups = (sx_hi - sx_lo + 4) >> 2;
        fits = groups <= s.max_groups && rows <= s.max_rows;
    }
    return vsd::C3Window{fits, sx_lo, sy_lo, rows, groups};
}

// the sampler's tile offset in bytes as place() forms it (vs_warp.hip): c0 once per lane, two fused multiply-adds per pixel
int sampler_offset(float flx, float fly, const vsd::C3Window& w, const Shape& sh) {
    const float sc = (float)sh.scale;
    const float c0 = -sc * (float)((w.sy_lo + sh.st.org) * sh.st.pitch + (w.sx_lo + sh.st.org));
    return (int)fmaf(fly, sc * (float)sh.st.pitch, fmaf(flx, sc, c0));
}

struct Verdict { bool sound, exact; };

// one tile's decision against the positions of its live pixels: Fx / Fy hold floor(Wx), floor(Wy) of the window's pixels (plain order) and
// Gx / Gy the same in the tabled order
Verdict judge(const vsd::C3Window& w, const Shape& sh, vsd::C3Tile t, vsd::C3Roi roi, const std::vector<float>& Fx, const std::vector<float>& Fy,
              const std::vector<float>& Gx, const std::vector<float>& Gy) {
    Verdict v{true, true};
    if (!w.fits) return v;
    const int x1 = std::min(t.x0 + t.tile_w, roi.w), y1 = std::min(t.y0 + t.tile_h, roi.h);
    const int lo = sh.st.org ? -1 : 0, hi = sh.st.org ? 2 : 1;          // the tap window about floor()
    for (int y = t.y0; y < y1; y++)
        for (int x = t.x0; x < x1; x++)
            for (int form = 0; form < 2; form++) {
                const float flx = (form ? Gx : Fx)[(size_t)y * roi.w + x], fly = (form ? Gy : Fy)[(size_t)y * roi.w + x];
                const double cx = (double)flx - w.sx_lo, cy = (double)fly - w.sy_lo;            // (positions below 10^6: exact)
                if (!(cx + lo >= 0 && cx + hi < 4.0 * w.groups && cy + lo >= 0 && cy + hi < (double)w.rows)) { v.sound = false; continue; }
                const long long want = (long long)sh.scale * (((long long)fly - w.sy_lo - sh.st.org) * sh.st.pitch + ((long long)flx - w.sx_lo - sh.st.org));
                if ((long long)sampler_offset(flx, fly, w, sh) != want) v.exact = false;
            }
    return v;
}

void positions(vsd::C3Params p, vsd::C3Roi roi, std::vector<float>& Fx, std::vector<float>& Fy, std::vector<float>& Gx, std::vector<float>& Gy) {
    const size_t n = (size_t)roi.w * roi.h;
    Fx.resize(n); Fy.resize(n); Gx.resize(n); Gy.resize(n);
    for (int y = 0; y < roi.h; y++)
        for (int x = 0; x < roi.w; x++) {
            const float fx = (float)(x + roi.x), fy = (float)(y + roi.y);
            const float A1x = p.A1 * fx, Bx = p.B * fx;
            const float Wx = A1x - p.B * fy + p.TX, Wy = Bx + p.A1 * fy + p.TY;                 // the sampler block, plain
            const float rb = p.B * fy, ra = p.A1 * fy;                                           // the row table's pair
            const float Vx = (A1x - rb) + p.TX, Vy = (Bx + ra) + p.TY;                            // the sampler block, tabled
            const size_t i = (size_t)y * roi.w + x;
            Fx[i] = floorf(Wx); Fy[i] = floorf(Wy); Gx[i] = floorf(Vx); Gy[i] = floorf(Vy);
        }
}

struct Tally { long tiles = 0, fits = 0, unsound = 0, inexact = 0, oversized = 0, old_fits = 0, old_unsound = 0, old_inexact = 0, far_cases = 0, far_inexact = 0; };

int run_grid() {
    // linear parts {A, B} (A1 = 1 + A): the first kFull of them meet every shift, the others the near ones
    std::vector<std::pair<double, double>> lin;
    auto turn = [&](double deg, double zoom) { const double a = deg * 3.14159265358979323846 / 180.0; lin.push_back({zoom * std::cos(a) - 1.0, zoom * std::sin(a)}); };
    turn(0, 1); turn(0.5, 1); turn(-0.9, 1); turn(0, 0.97); turn(0.1, 1.035); turn(180, 1); turn(5, 1); lin.push_back({-1 + 1e-9, 1e-9});
    const size_t kFull = lin.size();
    turn(0.2, 1); turn(1.2, 1); turn(-5, 1.1); turn(45, 1.4); turn(90, 1); turn(90, 0.5); turn(0, 0.5); turn(0, 0.83); turn(0, 1.5); turn(0, 2); turn(0.7, 0.99);
    lin.push_back({-2.0, 0.0});                 // mirror of both axes (A1 = -1)
    lin.push_back({-1.0, 0.0});                 // singular
    lin.push_back({-1 - 1e-9, -1e-9});          // near-singular
    lin.push_back({0.06, -0.0155});             // 16 rows of footprint, give or take (the 15.999 threshold's neighbourhood)
    lin.push_back({0.0155, 0.0});               // 64.98 columns
    lin.push_back({0.0159, 0.0});               // 65.0 columns
    // shifts: 0, +-1e4, +-1.9e5 .. +-2.4e5 in steps of 5000 (2^24 / 88 = 190650, / 81 = 207126, / 73 = 229825 lie inside), +-3e5, +-9.9e5, both sides of 1e6
    std::vector<double> far{0.3, 1e4 + 0.25, -1e4 - 0.25, 3e5 + 0.25, -3e5 - 0.25, 9.9e5 + 0.25, -9.9e5 - 0.25, 999900.25, -999900.25, 1000100.25, -1000100.25};
    for (double s = 1.9e5; s <= 2.4e5 + 1; s += 5000) { far.push_back(s + 0.25); far.push_back(-s - 0.25); }
    const std::vector<double> near{0.3, 1e4 + 0.25, -1e4 - 0.25, 3e5 + 0.25, -3e5 - 0.25};
    const vsd::C3Roi windows[] = {{0, 0, 130, 70}, {3, 5, 61, 14}, {65, 17, 65, 53}, {1, 33, 129, 1}};
    const double row_limit = 16777216.0;

    Tally tal[kNShapes];
    long compact_checked = 0, compact_bad = 0, printed = 0, cases = 0;
    std::vector<float> Fx, Fy, Gx, Gy;
    for (size_t li = 0; li < lin.size(); li++) {
        const std::vector<double>& sh = li < kFull ? far : near;
        for (size_t si = 0; si < sh.size(); si++)
            for (int axis = 0; axis < 3; axis++) {                   // the shift in x, in y, in both
                if (si == 0 && axis) continue;
                const double TXd = axis != 1 ? sh[si] : 0.3, TYd = axis != 0 ? sh[si] : -0.45;
                const float P4[4] = {(float)lin[li].first, (float)lin[li].second, (float)TXd, (float)TYd};
                const vsd::C3Params p{1.0f + P4[0], P4[1], P4[2], P4[3]};
                for (const vsd::C3Roi& roi : windows) {
                    cases++;
                    positions(p, roi, Fx, Fy, Gx, Gy);
                    for (int k = 0; k < kNShapes; k++) {
                        const Shape& S = kShapes[k];
                        float E4[4];
                        vsd::c3_extents(P4, 1, roi, kTileW, S.tile_h, E4);
                        const vsd::C3Extents E{E4[0], E4[1], E4[2], E4[3]};
                        const int compact = vsd::c3_compact_shape(E4, 1);
                        // a far-row case of this pitch: identity-like maps whose rows lie beyond 2^24 / pitch and below 10^6, columns inside the frame
                        const bool far_row = li == 0 && axis == 1 && std::fabs(TYd) * S.st.pitch > row_limit + 1e5 && std::fabs(TYd) < 9.99e5;
                        bool far_inexact = false;
                        for (int we = 0; we < 2; we++)
                            for (int y0 = 0; y0 < roi.h; y0 += S.tile_h)
                                for (int x0 = 0; x0 < roi.w; x0 += kTileW) {
                                    const vsd::C3Tile t{x0, y0, kTileW, S.tile_h};
                                    const vsd::C3Window nw = vsd::c3_tile_window(t, roi, p, we != 0, E, S.st);
                                    const vsd::C3Window od = replaced_form(t, roi, p, we != 0, E, S.st);
                                    const Verdict vn = judge(nw, S, t, roi, Fx, Fy, Gx, Gy), vo = judge(od, S, t, roi, Fx, Fy, Gx, Gy);
                                    Tally& T = tal[k];
                                    T.tiles++; T.fits += nw.fits; T.old_fits += od.fits;
                                    const bool over = nw.fits && !(nw.rows >= 1 && nw.rows <= S.st.max_rows && nw.groups >= 1 && nw.groups <= S.st.max_groups &&
                                                                   std::abs(nw.sx_lo) <= 1000004 && std::abs(nw.sy_lo) <= 1000004);
                                    T.unsound += !vn.sound; T.inexact += !vn.exact; T.oversized += over;
                                    T.old_unsound += !vo.sound; T.old_inexact += !vo.exact;
                                    far_inexact = far_inexact || !vo.exact;
                                    if ((!vn.sound || !vn.exact || over) && printed++ < 20)
                                        printf("BAD %s%s%s %s extents %d P %a %a %a %a window %d %d %d %d tile %d %d -> %d %d %d %d %d\n", vn.sound ? "" : "unsound ",
                                               vn.exact ? "" : "inexact ", over ? "oversized" : "", S.name, we, P4[0], P4[1], P4[2], P4[3], roi.x, roi.y, roi.w, roi.h, x0, y0,
                                               nw.fits, nw.sx_lo, nw.sy_lo, nw.rows, nw.groups);
                                    // where it is not refused outright the new form is the replaced one (the guard only ever refuses)
                                    if (nw.fits && !(od.fits && od.sx_lo == nw.sx_lo && od.sy_lo == nw.sy_lo && od.rows == nw.rows && od.groups == nw.groups)) {
                                        printf("BAD differs from the replaced form %s\n", S.name);
                                        T.oversized++;
                                    }
                                    // COMPACT: what the launcher concludes from the extents holds for every tile of the frame (both 20-row shapes)
                                    if (we && S.tabled && k >= 1 && compact >= k && nw.rows) {
                                        compact_checked++;
                                        if (nw.rows > S.st.max_rows || nw.groups > S.st.max_groups) {
                                            compact_bad++;
                                            printf("BAD compact %d: %s P %a %a %a %a tile %d %d rows %d groups %d\n", compact, S.name, P4[0], P4[1], P4[2], P4[3], x0, y0, nw.rows, nw.groups);
                                        }
                                    }
                                }
                        if (far_row) { tal[k].far_cases++; tal[k].far_inexact += far_inexact; }
                    }
                }
            }
    }
    long bad = compact_bad;
    for (int k = 0; k < kNShapes; k++) {
        const Tally& T = tal[k];
        printf("%s tiles %ld fits %ld | new unsound %ld inexact %ld oversized %ld | old fits %ld unsound %ld inexact %ld far_row_cases %ld far_row_inexact %ld\n", kShapes[k].name,
               T.tiles, T.fits, T.unsound, T.inexact, T.oversized, T.old_fits, T.old_unsound, T.old_inexact, T.far_cases, T.far_inexact);
        bad += T.unsound + T.inexact + T.oversized;
    }
    printf("COMPACT checked %ld bad %ld\nCASES %ld\nDONE\n", compact_checked, compact_bad, cases);
    return bad ? 1 : 0;
}

int run_cases() {
    char line[1024];
    long n = 0;
    while (fgets(line, sizeof line, stdin)) {
        char* q = line;
        double d[4];
        long v[8];
        bool ok = true;
        for (int k = 0; k < 4 && ok; k++) { char* e; d[k] = strtod(q, &e); ok = e != q; q = e; }
        for (int k = 0; k < 8 && ok; k++) { char* e; v[k] = strtol(q, &e, 10); ok = e != q; q = e; }
        if (!ok) { fprintf(stderr, "line %ld: twelve numbers expected\n", n + 1); return 2; }
        const int w = (int)v[0], h = (int)v[1];
        const vsd::C3Roi roi{(int)v[2], (int)v[3], (int)v[4], (int)v[5]};
        if (w < 1 || h < 1 || roi.w < 1 || roi.h < 1 || roi.x < 0 || roi.y < 0 || roi.x + roi.w > w || roi.y + roi.h > h || v[6] < 0 || v[6] >= kNShapes) {
            fprintf(stderr, "line %ld: window / shape\n", n + 1);
            return 2;
        }
        const Shape& S = kShapes[v[6]];
        const vs_transform t{d[0], d[1], d[2], d[3]};
        float P4[4], E4[4];
        vs_ul_params_warp(&t, w, h, P4);
        vsd::c3_extents(P4, 1, roi, kTileW, S.tile_h, E4);
        printf("E %a %a %a %a %d\n", E4[0], E4[1], E4[2], E4[3], vsd::c3_compact_shape(E4, 1));
        long tiles = 0;
        for (int y0 = 0; y0 < roi.h; y0 += S.tile_h)
            for (int x0 = 0; x0 < roi.w; x0 += kTileW, tiles++) {
                const vsd::C3Window nw = vsd::c3_tile_window(vsd::C3Tile{x0, y0, kTileW, S.tile_h}, roi, vsd::C3Params{1.0f + P4[0], P4[1], P4[2], P4[3]}, v[7] != 0,
                                                             vsd::C3Extents{E4[0], E4[1], E4[2], E4[3]}, S.st);
                printf("%d %d %d %d %d %d %d\n", x0, y0, nw.fits ? 1 : 0, nw.sx_lo, nw.sy_lo, nw.rows, nw.groups);
            }
        printf("END %ld\n", tiles);
        n++;
    }
    printf("DONE %ld\n", n);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "grid")) return run_grid();
    if (argc == 2 && !strcmp(argv[1], "cases")) return run_cases();
    fprintf(stderr, "usage: c3_window_test grid | cases < lines\n");
    return 2;
}
