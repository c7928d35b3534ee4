// The integer half of the aligner's run path (video_stabilizer_amd/csrc/vs_align_plan.hpp: level table, chunk sizing, frame bookkeeping, the
// fused solver's launch plan, result conversion) against the oracle where it has the same notion and against restatements written here.  Host
// only: built with the address and undefined-behaviour sanitizers together with csrc/vs_host.cpp and the oracle's sources
// (tests/test_align_plan_cpp.py).
#define VS_ALIGN_PLAN_UNIT
#include "../../video_stabilizer_amd/csrc/vs_align_plan.hpp"
#include "../../oracle/vs_oracle.h"

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

static int failures = 0;
static void expect(bool cond, const char* what, long a = 0, long b = 0, long c = 0) {
    if (!cond) { if (failures < 40) printf("FAIL %s (%ld %ld %ld)\n", what, a, b, c); failures++; }
}

static vs_aligner_params params(int min_w = 0, int min_h = 0, float fraction = 0.0f) {
    vs_aligner_params p;
    vs_aligner_params_default(&p);
    if (min_w) p.pyramid_min_width = min_w;
    if (min_h) p.pyramid_min_height = min_h;
    if (fraction > 0.0f) p.smallest_fraction = fraction;
    return p;
}

// ---- level table -------------------------------------------------------------------------------------
// a textured gray frame, shifted by `shift` pixels: enough structure for the oracle to walk every level
static std::vector<uint8_t> frame(int w, int h, int shift) {
    std::vector<uint8_t> f((size_t)w * h);
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int u = x + shift, v = y;
            f[(size_t)y * w + x] = (uint8_t)(128 + 50 * std::sin(u * 0.21) * std::cos(v * 0.17) + 40 * std::sin((u + 2 * v) * 0.043) + ((u * 7 + v * 13) % 11));
        }
    return f;
}

static void levels_against_oracle(int w, int h, const vs_aligner_params& p) {
    LevelTable t;
    expect(build_levels(w, h, p, &t) == VS_OK, "the size is accepted", w, h);
    vso_aligner_params q;
    vso_aligner_params_default(&q);
    q.pyramid_min_width = p.pyramid_min_width; q.pyramid_min_height = p.pyramid_min_height; q.smallest_fraction = p.smallest_fraction;
    vso_aligner* o = vso_aligner_create();
    vso_transform tr;
    const std::vector<uint8_t> f0 = frame(w, h, 0), f1 = frame(w, h, 1);
    vso_aligner_align_next(o, f0.data(), w, h, w, VSO_FMT_GRAY8, &q, &tr);
    vso_aligner_align_next(o, f1.data(), w, h, w, VSO_FMT_GRAY8, &q, &tr);
    const vso_align_debug* d = vso_aligner_debug(o);
    expect(d->levels == t.levels, "levels equal the oracle's", w, d->levels, t.levels);
    int reached = 0;
    for (int l = 0; l < t.levels && l < d->levels; l++) {
        int ow, oh, otx, oty, ots;
        expect(vso_aligner_level_dims(o, l, &ow, &oh, &otx, &oty, &ots) == 0, "the oracle has the level", l);
        const LevelDims& L = t.L[l];
        expect(L.w == ow && L.h == oh && L.tx == otx && L.ty == oty && L.ts == ots && L.nt == otx * oty, "level dimensions equal the oracle's", w, l);
        if (d->iterations[l] > 0) {
            reached++;
            expect(L.nsel == d->selected_x[l] && L.nsel == d->selected_y[l], "nsel equals the oracle's selected points", w, l, L.nsel);
        }
    }
    expect(reached >= 1, "the oracle's second frame reached a level", w, h);
    vso_aligner_destroy(o);
}

// the rule, restated: halve while both extents stay at or above the minimum; tiles of vs_tile_size; tables back to back
static void levels_against_rule(int w, int h, const vs_aligner_params& p) {
    LevelTable t;
    expect(build_levels(w, h, p, &t) == VS_OK, "the size is accepted", w, h);
    int lv = 1;
    while ((w >> lv) >= p.pyramid_min_width && (h >> lv) >= p.pyramid_min_height) lv++;
    expect(t.levels == lv, "levels follow the halving rule", w, t.levels, lv);
    size_t img = 0, lm = 0, jac = 0;
    int nt_max = 0;
    for (int l = 0; l < t.levels; l++) {
        const LevelDims& L = t.L[l];
        const int ww = w >> l, hh = h >> l, ts = vs_tile_size(ww, hh);
        expect(L.w == ww && L.h == hh && L.ts == ts && L.tx == ww / ts && L.ty == hh / ts && L.nt == (ww / ts) * (hh / ts), "level dimensions follow the rule", w, l);
        expect(L.nsel == (int)(size_t)((size_t)L.nt * p.smallest_fraction), "nsel is tiles x fraction, truncated", w, l);
        expect(L.img_off == img && L.lm_off == lm && L.jac_off == jac, "the level's tables start where the previous level's end", w, l);
        img += ((size_t)ww * hh + 255) / 256 * 256; lm += (size_t)4 * L.nt; jac += (size_t)8 * L.nt;
        nt_max = std::max(nt_max, L.nt);
    }
    expect(t.pyr_frame == img && t.lm_frame == (lm + 63) / 64 * 64 && t.jac_frame == (jac + 63) / 64 * 64 && t.nt_max == nt_max, "frame strides", w, h);
}

static void level_tests() {
    levels_against_oracle(64, 48, params(16, 12));
    levels_against_oracle(161, 121, params(20, 15));
    levels_against_oracle(320, 240, params());
    levels_against_oracle(640, 360, params());
    levels_against_oracle(320, 240, params(0, 0, 0.25f));
    levels_against_oracle(320, 240, params(0, 0, 1.0f));
    for (float f : {0.25f, 0.8f, 1.0f}) {
        levels_against_rule(64, 48, params(16, 12, f));
        levels_against_rule(161, 121, params(20, 15, f));
        levels_against_rule(320, 240, params(0, 0, f));
        levels_against_rule(1920, 1080, params(256, 0, f));
        levels_against_rule(3840, 2160, params(256, 0, f));
    }
    LevelTable t;
    expect(build_levels(64, 48, params(16, 12), &t) == VS_OK && t.levels == 3 && t.L[0].ts == 2, "64 x 48: three levels, tile size 2", t.levels, t.L[0].ts);
    expect(build_levels(161, 121, params(20, 15), &t) == VS_OK && t.L[1].w == 80 && t.L[1].h == 60 && t.L[2].w == 40 && t.L[2].h == 30, "odd halving");
    expect(build_levels(3840, 2160, params(256), &t) == VS_OK && t.L[0].nt == 20736 && t.L[0].ts == 20, "4K level 0: 20 736 tiles of 20", t.L[0].nt, t.L[0].ts);
    expect(t.L[t.levels - 1].w == 480 && t.L[t.levels - 1].h == 270, "4K: the coarsest level is 480 x 270");
    expect(build_levels(1920, 1080, params(256), &t) == VS_OK && t.L[t.levels - 1].w == 480 && t.L[t.levels - 1].h == 270, "1080p: the coarsest level is 480 x 270");
    // set_fraction: nsel follows the current parameters, nothing else moves
    LevelTable u = t;
    u.set_fraction(0.5f);
    for (int l = 0; l < u.levels; l++)
        expect(u.L[l].nsel == u.L[l].nt / 2 && u.L[l].nt == t.L[l].nt && u.L[l].w == t.L[l].w && u.L[l].img_off == t.L[l].img_off, "set_fraction touches nsel only", l);
    expect(u.levels == t.levels && u.nt_max == t.nt_max && u.pyr_frame == t.pyr_frame, "set_fraction touches nsel only");
    // refusals: the parent's code, and no table left behind
    LevelTable mark, keep;
    memset((void*)&mark, 0xA5, sizeof mark);
    memcpy((void*)&keep, (const void*)&mark, sizeof keep);
    expect(build_levels(1024, 16, params(1, 1), &mark) == VS_ERR_UNSUPPORTED && strstr(vs_last_error(), "levels below 4x4"), "a level below 4 x 4 is refused");
    expect(build_levels(64, 48, params(32, 24), &mark) == VS_ERR_UNSUPPORTED && strstr(vs_last_error(), "gives 2 pyramid levels"), "fewer than 3 levels are refused");
    expect(build_levels(70000, 1000, params(), &mark) == VS_ERR_UNSUPPORTED && strstr(vs_last_error(), "65535"), "more than 65 535 px is refused");
    expect(memcmp(&mark, &keep, sizeof keep) == 0, "a refusal leaves no table behind");
}

// ---- bookkeeping ---------------------------------------------------------------------------------------
static void bookkeeping_tests() {
    ChunkFrames fr;                                              // one value, reassigned: what the handle does
    for (long long seq0 : {0LL, 1LL, 2LL, 7LL})
        for (int clip_len = 0; clip_len <= 5; clip_len++)
            for (int n = 1; n <= 12; n++) {
                fr.assign(seq0, clip_len, n);
                std::vector<int> pairs;
                std::set<int> key;
                for (int i = 0; i < n; i++) {
                    const long long g = clip_len > 0 ? i % clip_len : seq0 + i;
                    expect(fr.g(i) == g, "sequence index", seq0, clip_len, i);
                    expect(fr.first(i) == (g == 0), "first frame of a sequence", seq0, clip_len, i);
                    if (g >= 1) pairs.push_back(i);
                    if (g & 1) key.insert(i);
                }
                expect(fr.pair_frame == pairs && fr.n_pairs() == (int)pairs.size(), "a pair exists iff g >= 1", seq0, clip_len, n);
                for (int q = 0; q < fr.n_pairs(); q++) {
                    const int i = pairs[(size_t)q];
                    const bool cur_is_key = (fr.g(i) & 1) != 0;
                    const PairDesc d = fr.desc(q);
                    // slots (i, i + 1) hold frames (g - 1, g): the key slot is the odd one
                    expect(d.key_slot == (cur_is_key ? i + 1 : i) && d.tmpl_slot == (cur_is_key ? i : i + 1), "key slot: the odd frame of the two", seq0, clip_len, i);
                    expect(fr.negate(q) == cur_is_key, "negate iff the current frame is the keyframe", seq0, clip_len, i);
                }
                std::multiset<int> covered;
                for (const std::pair<int, int>& r : fr.key_runs) {
                    expect(r.second >= 1, "no empty run", seq0, clip_len, n);
                    for (int k = 0; k < r.second; k++) covered.insert(r.first + 2 * k);
                }
                expect(covered.size() == key.size() && std::equal(covered.begin(), covered.end(), key.begin()), "the runs cover every odd-g frame once, at stride 2", seq0, clip_len, n);
                if (clip_len == 1) expect(fr.n_pairs() == 0 && fr.key_runs.empty(), "clips of one frame: no pair, every frame first", n);
            }
}

// ---- chunk sizing ----------------------------------------------------------------------------------------
static void sizing_tests() {
    const size_t small = 4096;                                   // a pyramid small enough for the 1024-frame clamp
    int m = 0;
    expect(max_chunk_frames(small, 0, &m) == VS_OK && m == 1024, "the chunk is clamped to 1024 frames", m);
    expect(max_chunk_frames((size_t)1 << 30, 0, &m) == VS_OK && m == 6, "6 GiB of pyramids", m);
    expect(max_chunk_frames((size_t)4 << 30, 0, &m) == VS_OK && m == 2, "at least 2 frames", m);
    expect(max_chunk_frames(0, 0, &m) == VS_OK && m == 1024, "no table yet", m);
    expect(max_chunk_frames(small, 10, &m) == VS_OK && m == 1020, "whole clips: 1020 frames for clips of 10", m);
    m = -7;
    expect(max_chunk_frames(small, 1025, &m) == VS_ERR_UNSUPPORTED && m == -7 && strstr(vs_last_error(), "clips of 1025 frames exceed the 1024-frame chunk"),
           "a clip longer than the chunk is refused");
    for (size_t pyr : {small, (size_t)7 << 20, (size_t)1 << 30})
        for (int clip_len : {0, 1, 3, 10, 1024})
            for (int n : {1, 1024, 1025, 1030}) {
                const size_t by_mem = ((size_t)6 << 30) / pyr;
                int want = (int)(by_mem > 1024 ? 1024 : by_mem < 2 ? 2 : by_mem);
                const int r = max_chunk_frames(pyr, clip_len, &m);
                if (clip_len > want) { expect(r == VS_ERR_UNSUPPORTED, "refused", (long)pyr, clip_len); continue; }
                if (clip_len > 0) want = want / clip_len * clip_len;
                expect(r == VS_OK && m == want, "max_chunk restated", (long)pyr, clip_len, m);
                for (size_t step : {(size_t)1, (size_t)9216, (size_t)6220800}) {
                    for (size_t ingest : {(size_t)1, (size_t)3 * 9216, (size_t)192 << 20}) {
                        size_t hw = ingest / step;
                        if (hw < 4) hw = 4;
                        if (hw > (size_t)m) hw = (size_t)m;
                        int hc = (int)hw;
                        if (clip_len > 0) hc = hc / clip_len * clip_len < clip_len ? clip_len : hc / clip_len * clip_len;
                        const int host = vsi::host_chunk_frames(m, ingest, step, clip_len);
                        expect(host == hc && host >= 1, "host_chunk restated", (long)step, (long)ingest, host);
                        expect(host <= m, "an upload fits a chunk", host, m);
                    }
                }
                // the chunks of a call (chunk_count / chunk_span: what both cutting loops of vs_engine.hip walk) tile [0, n) whatever n
                // is; a call of whole clips (the API takes no other: n = n_clips * clip_len) gets whole clips in every chunk
                for (int total : {n, clip_len > 0 ? (n + clip_len - 1) / clip_len * clip_len : n})
                    for (int step : {m, vsi::host_chunk_frames(m, (size_t)3 * 9216, 9216, clip_len)}) {
                        const bool whole = clip_len == 0 || total % clip_len == 0;
                        int covered = 0;
                        for (int k = 0; k < chunk_count(total, step); k++) {
                            const ChunkSpan c = chunk_span(total, step, k);
                            expect(c.off == covered && c.len >= 1 && c.len <= step, "a chunk follows the previous one", c.off, c.len, step);
                            if (whole) expect(c.off % std::max(1, clip_len) == 0 && c.len % std::max(1, clip_len) == 0, "a chunk holds whole clips", c.off, c.len, clip_len);
                            covered += c.len;
                        }
                        expect(covered == total, "the chunks tile the call", total, step);
                    }
            }
    expect(max_chunk_frames(small, 10, &m) == VS_OK && (1030 - m) == 10, "1030 frames in clips of 10: chunks of 1020 and 10", m);
}

// ---- the solver's launch plan ---------------------------------------------------------------------------
// The rules of the fused launch as the run path had them before they became plan_solver, numbers written out.
struct Want {
    bool direct, use_host, cores;
    int pipeline, group, threads, build;
    size_t dyn, selbuf_pair, selbuf_bytes, recs_pair;
};
static Want restate(const LevelTable& t, int n_pairs, int cap, const vs_aligner_params& p, int select_mode, int batch_mode, int cu_count, bool coop_ok,
                    const SolverKnobs& k) {
    Want w{};
    const size_t nt_max = (size_t)t.nt_max, lds = 150 * 1024;
    w.direct = n_pairs <= 16 && !p.phase_correlate && select_mode != VS_SELECT_STL_HOST && nt_max <= 26000;
    w.use_host = select_mode == VS_SELECT_STL_HOST || nt_max > 26000;
    w.pipeline = k.pipeline >= 0 ? k.pipeline : (n_pairs <= 128 ? 1 : 0);
    w.recs_pair = 2 * nt_max * 28;
    w.group = 1; w.threads = 512; w.build = 0;
    if (w.use_host) return w;
    auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    size_t dyn = up16(nt_max * (nt_max * 12 <= lds ? 12 : 6));
    const LevelDims& c = t.L[t.levels - 1];
    const size_t img = (size_t)c.w * c.h + 8;
    if (img <= lds) dyn = std::max(dyn, up16(img));
    if (up16(img) + (size_t)c.nt * 12 <= lds) dyn = std::max(dyn, up16(up16(img) + (size_t)c.nt * 12));
    dyn = std::max<size_t>(dyn, 512);
    if (coop_ok && n_pairs <= 128 && t.L[0].nt >= 4096) {
        if (k.helpers >= 0) w.group = std::max(1, std::min(k.helpers, 16));
        else w.group = std::max(1, std::min(16, cu_count / n_pairs));
    }
    const bool small_wg = nt_max <= 26000;
    w.cores = small_wg && nt_max <= 128 * 256 && (k.coresident >= 0 ? k.coresident != 0 : (batch_mode == VS_BATCH_SHARED && n_pairs >= 32));
    w.selbuf_pair = (nt_max * 6 + 255) / 256 * 256;
    if (w.cores) {
        w.group = 1;
        dyn = 16;
        bool need_global = false;
        for (int l = 0; l < t.levels; l++) {
            const size_t nt = (size_t)t.L[l].nt;
            const size_t need = up16(nt <= 32 * 128 && nt * 12 <= 32 * 1024 ? nt * 12 : nt * 6);
            if (need <= 32 * 1024) dyn = std::max(dyn, need); else need_global = true;
        }
        dyn = std::max<size_t>(dyn, 512);
        w.selbuf_bytes = need_global ? w.selbuf_pair * (size_t)std::max(cap, n_pairs) : 256;
    }
    w.build = w.cores ? 2 : (small_wg ? 0 : 1);
    w.threads = w.cores ? 256 : (small_wg ? 512 : 1024);
    w.dyn = dyn;
    return w;
}

static void plan_tests() {
    LevelTable qvga, hd, uhd;
    expect(build_levels(320, 240, params(), &qvga) == VS_OK && build_levels(1920, 1080, params(256), &hd) == VS_OK &&
           build_levels(3840, 2160, params(256), &uhd) == VS_OK, "the three sizes");
    std::vector<SolverKnobs> knobs(1);                            // all unset, then each knob at its override values
    auto with = [&](int SolverKnobs::*field, int v) { SolverKnobs k; k.*field = v; knobs.push_back(k); };
    with(&SolverKnobs::pipeline, 0); with(&SolverKnobs::pipeline, 1);
    with(&SolverKnobs::stall_helpers, 1);
    with(&SolverKnobs::select_depth, 3);
    with(&SolverKnobs::helpers, 0); with(&SolverKnobs::helpers, 1); with(&SolverKnobs::helpers, 4); with(&SolverKnobs::helpers, 99);
    with(&SolverKnobs::coresident, 0); with(&SolverKnobs::coresident, 1);
    { SolverKnobs k; k.poll = false; knobs.push_back(k); }
    long cases = 0;
    for (const LevelTable* t : {&qvga, &hd, &uhd})
        for (int n_pairs : {1, 16, 17, 31, 32, 128, 129, 300})
            for (int batch_mode : {VS_BATCH_EXCLUSIVE, VS_BATCH_SHARED})
                for (int select_mode : {VS_SELECT_STL_HOST, VS_SELECT_DEVICE, VS_SELECT_STABLE})
                    for (int phase : {0, 1})
                        for (int cu_count : {256, 64})
                            for (bool coop_ok : {true, false})
                                for (size_t ki = 0; ki < knobs.size(); ki++) {
                                    const SolverKnobs& k = knobs[ki];
                                    vs_aligner_params p = params();
                                    p.phase_correlate = phase;
                                    p.threshold = 0.03125; p.max_displacement = 24.0; p.max_iters = 17;
                                    const int cap = std::max(n_pairs, 40);
                                    const SolverPlan s = plan_solver(*t, n_pairs, cap, p, select_mode, batch_mode, cu_count, coop_ok, k);
                                    const Want w = restate(*t, n_pairs, cap, p, select_mode, batch_mode, cu_count, coop_ok, k);
                                    cases++;
                                    expect(s.direct == w.direct && s.use_host == w.use_host && s.cores == w.cores, "direct / use_host / cores", t->nt_max, n_pairs, (long)ki);
                                    expect(s.group == w.group && s.threads == w.threads && s.build == w.build, "group / threads / build", t->nt_max, n_pairs, (long)ki);
                                    expect(s.dyn == w.dyn && s.selbuf_pair == w.selbuf_pair && s.selbuf_bytes == w.selbuf_bytes && s.recs_pair == w.recs_pair,
                                           "dyn / selbuf / recs", t->nt_max, n_pairs, (long)ki);
                                    expect(s.gp.threshold == p.threshold && s.gp.max_displacement == p.max_displacement && s.gp.max_iters == p.max_iters &&
                                           s.gp.pipeline == w.pipeline && s.gp.stall_helpers == k.stall_helpers && s.gp.sel_depth_cap == k.select_depth &&
                                           s.gp.sel_stable == (select_mode == VS_SELECT_STABLE ? 1 : 0), "the solver's parameters", t->nt_max, n_pairs, (long)ki);
                                    // anchors from the comments of the code
                                    expect(s.direct == (n_pairs <= 16 && !phase && select_mode != VS_SELECT_STL_HOST && t->nt_max <= kSelectCap), "direct", n_pairs);
                                    if (t == &qvga) expect(s.group == 1, "320 x 240: no helpers", n_pairs, (long)ki);
                                    if (s.cores) expect(s.group == 1 && s.threads == 256, "the small-footprint build runs without helpers", n_pairs);
                                    if (k.coresident < 0) expect(s.cores == (!s.use_host && batch_mode == VS_BATCH_SHARED && n_pairs >= 32),
                                                                 "the small-footprint build: from 32 pairs in shared mode", n_pairs, batch_mode);
                                    if (!s.use_host) expect(s.dyn >= 512 && s.dyn % 16 == 0 && s.dyn <= 150 * 1024, "dynamic LDS within the bound", (long)s.dyn);
                                    if (!s.use_host && !s.cores && coop_ok && k.helpers < 0 && t != &qvga && n_pairs <= 128)
                                        expect(s.group == std::max(1, std::min(16, cu_count / n_pairs)), "helpers: 16 per pair while the launch stays within the chip", n_pairs, cu_count);
                                }
    expect(cases == 3L * 8 * 2 * 3 * 2 * 2 * 2 * 12, "every combination ran", cases);
    // side-by-side selection (12 B per tile): every level at 1080p, every level but the finest at 4K
    for (int l = 0; l < hd.levels; l++) expect((size_t)hd.L[l].nt * 12 <= kLdsBound, "1080p: both sets side by side", l);
    expect((size_t)uhd.L[0].nt * 12 > kLdsBound && (size_t)uhd.L[0].nt * 6 <= kLdsBound, "4K level 0: one set at a time");
    for (int l = 1; l < uhd.levels; l++) expect((size_t)uhd.L[l].nt * 12 <= kLdsBound, "4K above level 0: both sets side by side", l);
    const SolverKnobs none;
    const vs_aligner_params p = params();
    expect(plan_solver(hd, 1, 1, p, VS_SELECT_DEVICE, VS_BATCH_EXCLUSIVE, 256, true, none).dyn >= (size_t)hd.nt_max * 12, "1080p: 12 B per tile of LDS");
    const size_t dyn4k = plan_solver(uhd, 1, 1, p, VS_SELECT_DEVICE, VS_BATCH_EXCLUSIVE, 256, true, none).dyn;
    expect(dyn4k >= (size_t)uhd.nt_max * 6 && dyn4k < (size_t)uhd.nt_max * 12, "4K: 6 B per tile of LDS", (long)dyn4k);
    expect(hd.L[0].nt >= kCoopMinTiles && qvga.L[0].nt < kCoopMinTiles, "helpers from 4096 tiles at level 0", hd.L[0].nt, qvga.L[0].nt);
    expect(kPointRecBytes == 28 && recs_pair_bytes(100) == 5600, "28 bytes per selected point");
    // the knobs come from the environment, once
    const SolverKnobs& k = solver_knobs();
    expect(k.pipeline == -1 && k.stall_helpers == 0 && k.select_depth == 5 && k.helpers == 4 && k.coresident == 0 && !k.poll, "knobs as set in main");
    setenv("VS_GN_HELPERS", "9", 1);
    expect(solver_knobs().helpers == 4, "the knobs are read once per process");
}

// ---- result conversion ---------------------------------------------------------------------------------------
static void conversion_tests() {
    LevelTable t;
    expect(build_levels(320, 240, params(), &t) == VS_OK && t.levels >= 3, "table");
    PairState st;
    memset(&st, 0, sizeof st);
    st.T[0] = 0.01; st.T[1] = -0.02; st.T[2] = 3.5; st.T[3] = -1.25;
    st.status = 1;
    for (int l = 1; l < t.levels; l++) {                          // level 0 is left unreached: 0 iterations
        st.iterations[l] = l + 2; st.condition[l] = 10.0 * l;
        for (int c = 0; c < 4; c++) st.level_T[l][c] = 0.001 * (l * 4 + c + 1);
    }
    st.level_T[0][2] = 99.0;                                        // (must not show: the level ran no iteration)
    const vs_transform fwd{st.T[0], st.T[1], st.T[2], st.T[3]};
    for (int failed : {0, 1})
        for (long long g : {1LL, 2LL, 7LL, 8LL}) {
            st.status = failed ? 0 : 1; st.fail_reason = failed ? 2 : 0; st.fail_level = failed ? 1 : 0;
            vs_align_info inf, want;
            memset(&inf, 0, sizeof inf);
            inf.levels = t.levels;
            want = inf;
            vs_transform out{9, 9, 9, 9};
            int32_t status = 0;
            const int its = convert_result(st, g, t, &inf, &out, &status);
            want.status = st.status; want.fail_reason = st.fail_reason; want.fail_level = st.fail_level;
            int sum = 0;
            for (int l = 1; l < t.levels; l++) {
                want.iterations[l] = l + 2; want.condition[l] = 10.0 * l; sum += l + 2;
                want.selected_x[l] = want.selected_y[l] = t.L[l].nsel;
                want.level_transform[l] = vs_transform{st.level_T[l][0], st.level_T[l][1], st.level_T[l][2], st.level_T[l][3]};
            }
            expect(memcmp(&inf, &want, sizeof want) == 0 && its == sum, "the record: reached levels only", failed, (long)g);
            const vs_transform t_want = (!failed && (g & 1) == 0) ? vs_transform_inverse(&fwd) : fwd;
            expect(memcmp(&out, &t_want, sizeof t_want) == 0, "inverse for even g on success only; the estimate as it stands otherwise", failed, (long)g);
            expect(status == (failed ? 0 : 1), "status", failed, (long)g);
        }
    expect(sizeof(PairState) == 32 + 16 + 16 * 4 + 16 * 8 + 16 * 32 && offsetof(PairState, pad) == 44 && offsetof(PairState, level_T) == 240, "PairState's layout",
           (long)sizeof(PairState));
}

int main() {
    setenv("VS_GN_HELPERS", "4", 1); setenv("VS_GN_SELECT_DEPTH", "5", 1); setenv("VS_GN_CORESIDENT", "0", 1); setenv("VS_GN_POLL", "0", 1);
    unsetenv("VS_GN_PIPELINE"); unsetenv("VS_GN_STALL_HELPERS");
    level_tests();
    bookkeeping_tests();
    sizing_tests();
    plan_tests();
    conversion_tests();
    if (failures) { printf("%d FAILURE(S)\n", failures); return 1; }
    printf("ALL PASS\n");
    return 0;
}
