"""The inputs of tests/test_align_state_gpu.py, proved without a GPU: the stage-wise reference equals what oracle.Aligner itself holds, the
boundary palette notices a rounding constant or a split weight that is off by one, the size and case tables reach every tile size and every
route of the ingest and pyramid kernels, the hostile keyframes do what their names say, and the comparison the GPU module relies on reports a
single damaged byte, keypoint or Jacobian bit."""
import copy

import numpy as np
import pytest

import _align_state as S
from oracle import oracle as O


# ---- reference_state against the reference restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,w,h,params", [(O.FMT_GRAY8, 203, 191, {}), (O.FMT_BGR8, 129, 33, S.TINY), (O.FMT_BGR8, 322, 246, {}),
                                             (O.FMT_BGR10, 494, 99, S.TINY), (O.FMT_BGR12, 150, 130, S.TINY), (O.FMT_BGR16_FULL, 133, 67, S.TINY)])
def test_reference_state_is_what_the_oracle_aligner_holds(fmt, w, h, params):
    frames = [S.noise(w, h, 40 + k, fmt) for k in range(2)]
    al = O.Aligner(**params)
    for f in frames:
        al.align_next(f, fmt=fmt)
    levels = al.debug().levels
    assert levels >= 3
    held = [[], []]
    for l in range(levels):
        d = al.level(l)
        for k in (0, 1):            # frame k lives in image k & 1; the tables are those of frame 1, the keyframe
            held[k].append({"w": d["w"], "h": d["h"], "ts": d["ts"], "img": d["img"][k & 1], "argmax": d["argmax"], "jac": d["jac"]})
    want = [S.reference_state(f, fmt, **params) for f in frames]
    assert S.call_diffs(held, want, keyframes=[1]) == []
    assert [(e["w"], e["h"], e["ts"]) for e in want[0]] == S.level_dims(w, h, **params)


# ---- the palette ----------------------------------------------------------------------------------------------------------------------------
def test_8_bit_palette_holds_every_boundary_colour():
    """exhaustive over the 2^24 colours: 2728 of them sit exactly on the rounding boundary (residue 0), none sits one below it -- the largest
    residue that occurs is 32764, so rounding constants 16384 .. 16387 are one and the same function of an 8-bit colour"""
    p = S.boundary_palette(8)
    b, g, r = np.meshgrid(*(np.arange(256, dtype=np.int64),) * 3, indexing="ij")
    every = np.stack([b.ravel(), g.ravel(), r.ravel()], 1)
    res = S.residue(every, 8)
    top = int(res.max())
    assert top == 32764
    for side, value in (("above", 0), ("below", top)):
        want = {tuple(c) for c in every[res == value]}
        assert {tuple(c) for c in p[side]} == want
    assert len(p["above"]) == 2728
    for d in (1, 2, 3):
        assert np.array_equal(S.gray_numpy(every, 8, rounding=16384 + d), S.gray_numpy(every, 8))


@pytest.mark.parametrize("bits", [8, 10, 12, 16])
def test_palette_notices_a_rounding_constant_that_is_off(bits):
    """16384 - 1 changes the gray of a palette colour at every depth; 16384 + 1 does so at 10, 12 and 16 bits.  At 8 bits no colour at all
    can tell 16384 + 1 from 16384 (the test above); there the palette notices the smallest increase any colour notices, + 4."""
    cols = S.palette_colours(bits)
    assert cols.min() >= 0 and cols.max() <= (0xFFFF if bits > 8 else 0xFF)
    p = S.boundary_palette(bits)
    assert max(p[k].max() for k in ("above", "below", "corners")) <= (1 << bits) - 1
    want = S.gray_numpy(cols, bits)
    up = 4 if bits == 8 else 1
    lower, higher = S.gray_numpy(cols, bits, rounding=16384 - 1), S.gray_numpy(cols, bits, rounding=16384 + up)
    assert (lower != want).any() and (lower <= want).all()
    assert (higher != want).any() and (higher >= want).all()
    # the corners and the values above the format's maximum clamp like the oracle clamps them
    if len(p["over"]):
        assert (S.gray_numpy(p["over"], bits) == 255).sum() >= 6 and int(p["over"].max()) == 0xFFFF
    frame = cols.reshape(1, -1, 3).astype(S.fmt_dtype(S.FMT_OF_BITS[bits]))
    assert np.array_equal(O.bgr_to_gray(frame, shift_to_8=bits - 8).ravel(), want)


def test_8_bit_palette_notices_a_split_weight_lowered_by_one():
    """the u8 group route computes byte 2 of B*b + G*g + R*r + 32768 with b, g, r = the doubled weights in the split form
    (w >> 7) * 256 + 2 * (w & 127): the form is the formula, and any one weight one too small changes a palette gray"""
    cols = S.palette_colours(8)
    want = S.gray_numpy(cols, 8)
    assert np.array_equal(S.gray_split_numpy(cols), want)
    for ch in range(3):
        assert (S.gray_split_numpy(cols, lowered=ch) != want).any(), ch


def test_palette_frame_draws_every_colour():
    for bits in (8, 10):
        f = S.palette_frame(264, 70, bits, seed=3)
        assert f.shape == (70, 264, 3) and f.dtype == S.fmt_dtype(S.FMT_OF_BITS[bits])
        assert {tuple(c) for c in f.reshape(-1, 3).tolist()} == {tuple(c) for c in S.palette_colours(bits).tolist()}
        assert not np.array_equal(f, S.palette_frame(264, 70, bits, seed=4))


# ---- the tables of the GPU module --------------------------------------------------------------------------------------------------------------
def test_keyframe_sizes_reach_every_tile_size_and_the_partly_filled_ends():
    all_ts = set(range(2, 21, 2))
    dims = [S.level_dims(w, h) for w, h in S.KEYFRAME_SIZES]
    assert {lv[0][2] for lv in dims} == all_ts                       # at level 0 alone, where the hostile content is
    assert {ts for lv in dims for _, _, ts in lv} == all_ts
    assert all(len(lv) >= 3 for lv in dims)
    last_strip, last_group = 0, 0
    for (w, h), lv in zip(S.KEYFRAME_SIZES, dims):
        ts = lv[0][2]
        assert w % ts and h % ts and max(w, h) <= 664, (w, h, ts)
        tx, ty, tpw = w // ts, h // ts, S.tiles_per_wave(ts)
        last_strip += tx % tpw != 0
        last_group += (-(-tx // tpw) * ty) % 4 != 0
    assert last_strip and last_group
    kinds = [k for call in S.KEYFRAME_CALLS for k in call]
    assert set(kinds) == set(S.KINDS) | {"noise"} and all(a != b for a, b in S.KEYFRAME_CALLS)


def test_batch_sizes_reach_the_strip_band_and_tile_edges():
    dims = {s: S.level_dims(*s, **S.TINY) for s in S.BATCH_SIZES}
    assert {w % 4 for w, _ in S.BATCH_SIZES} == {0, 1, 2, 3}
    assert {lv[1][0] for lv in dims.values()} >= {247, 248, 249}                      # the 248-column strip of vs_k_pyr_down_rows
    heights = {h for lv in dims.values() for _, h, _ in lv[1:]}
    assert any(h % 16 == 0 for h in heights) and any(h % 16 == 1 and h > 16 for h in heights)
    assert {(127, 31), (128, 32), (129, 33)} <= set(S.BATCH_SIZES) and any(w <= 128 for w, _ in S.BATCH_SIZES)
    assert any(4 <= lv[-1][0] <= 7 for lv in dims.values()) and any(lv[-1][0] == 4 for lv in dims.values())
    assert all(3 <= len(lv) <= 16 and lv[-1][0] >= 4 and lv[-1][1] >= 4 and max(s) <= 660 for s, lv in dims.items())
    assert {S.pyr_route(sum(ns) if clips else n) for _, clips, ns in S.BATCH_CALLS for n in ns} == {4, 16}
    assert max(n for _, _, ns in S.BATCH_CALLS for n in ns) <= 8
    # the second call of "batch3then4" starts at an odd sequence index: its first keyframe is its frame 0
    assert S.key_frames(4, seq0=3) == [0, 2] and S.key_frames(6) == [1, 3, 5] and S.key_frames(6, clip_len=3) == [1, 4]
    assert S.key_frames(8, clip_len=4) == [1, 3, 5, 7]


@pytest.mark.parametrize("fmt", [O.FMT_BGR8, O.FMT_BGR10])
def test_route_cases_reach_every_route(fmt):
    cases = [c for c in S.ROUTE_CASES if c[0] == fmt]
    routes = {r for c in cases for dev in (False, True) for r in S.route_case_routes(c, dev)}
    assert {r.kind for r in routes} == {"byte", "group"}
    group = {r for r in routes if r.kind == "group"}
    assert any(not r.interior and not r.one_column for r in group)                    # rim tiles only
    assert any(r.interior for r in group) and any(r.one_column for r in group)
    assert {r.wmod4 for r in group} == {0, 1, 2, 3}
    assert {r.wmod4 for r in routes if r.kind == "byte"} >= {0, 3}
    assert not any(r.interior for r in routes if r.wmod4 or r.kind == "byte")
    assert {c[6] for c in cases} == {0, 1, 2, 3}                                      # base offsets, in elements
    # device frames at an odd byte offset leave the group route; host frames are copied to an aligned start and keep it
    assert any(S.route_case_routes(c, True)[0].kind == "byte" and S.route_case_routes(c, False)[0].kind == "group" for c in cases if c[6])
    # the route changes between the frames of one launch
    assert any(len({r.kind for r in S.route_case_routes(c, False)}) == 2 and S.route_case_routes(c, False)[0].kind == "group" for c in cases)
    for c in cases:
        pitch, frame_pitch, _ = S.route_case_layout(c)
        assert pitch >= c[1] * 3 and frame_pitch >= (c[2] - 1) * pitch + c[1] * 3 and c[3] <= 4


def test_ingest_route_rules():
    R = S.ingest_route
    assert R(3, 40, 1, 12, 0, 480, 0).kind == "byte"                                  # w < 4
    assert R(479, 71, 1, 1437, 0, 0, 0).kind == "byte" and R(479, 71, 1, 1452, 0, 0, 0) == ("group", False, False, 3)
    assert R(260, 65, 1, 780, 0, 0, 0).interior and not R(256, 65, 1, 768, 0, 0, 0).interior and not R(260, 64, 1, 780, 0, 0, 0).interior
    assert R(128, 96, 2, 384, 0, 0, 0).one_column and not R(129, 96, 2, 388, 0, 0, 0).one_column
    assert R(131, 67, 2, 393, 0, 0, 0).kind == "byte" and R(131, 67, 2, 394, 0, 0, 0).kind == "group"
    assert R(132, 67, 1, 396, 0, 67 * 396 + 2, 1).kind == "byte" and R(132, 67, 1, 396, 0, 67 * 396 + 2, 2).kind == "group"
    assert R(132, 67, 2, 396, 2, 67 * 396, 0).kind == "byte" and R(132, 67, 2, 396, 0, 67 * 396, 1).kind == "group"
    assert [S.pyr_route(n) for n in (1, 3, 4, 5, 6)] == [4, 4, 4, 16, 16]


def test_palette_cases_meet_both_routes_with_and_without_interior_tiles():
    for bits in (8, 10, 12, 16):
        es = 1 if bits == 8 else 2
        routes = [S.ingest_route(w, h, es, pitch or w * 3, 0, h * (pitch or w * 3), 0) for b, w, h, pitch in S.palette_cases() if b == bits]
        assert len(routes) == 4 and {r.kind for r in routes} == {"byte", "group"}
        assert any(r.interior for r in routes) and any(r.kind == "group" and not r.interior for r in routes)
        assert any(r.kind == "byte" and r.wmod4 == 0 for r in routes) and any(r.kind == "byte" and r.wmod4 for r in routes)


def test_embed_puts_frames_where_the_pitches_say():
    frames = S.noise(5, 3, 1, O.FMT_BGR10)[None].repeat(2, 0).copy()
    frames[1] += 1
    buf, off = S.embed(frames, 17, 60, 3, 0xFFFF)
    assert off == 3 and buf.dtype == np.uint16 and len(buf) == 3 + 60 + 2 * 17 + 15 + S.TAIL
    mask = np.ones(len(buf), bool)
    for i in range(2):
        for r in range(3):
            s = 3 + i * 60 + r * 17
            assert np.array_equal(buf[s:s + 15], frames[i, r].ravel())
            mask[s:s + 15] = False
    assert (buf[mask] == 0xFFFF).all()


# ---- the hostile keyframes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [S.KEYFRAME_SIZES[0], S.KEYFRAME_SIZES[1], S.KEYFRAME_SIZES[4], S.KEYFRAME_SIZES[9]])
def test_hostile_keyframes_do_what_they_say(w, h):
    ts = O.tile_size(w, h)
    tx, ty = w // ts, h // ts

    def level0(kind):
        f = S.keyframe_hostile(w, h, kind, seed=5)
        assert f.shape == (h, w) and f.dtype == np.uint8
        gx, gy = O.grad_xy(f)
        _, lmx, lmy = O.grad_argmax(gx, gy, ts)
        return f, (np.abs(gx), np.abs(gy)), (lmx, lmy)

    def tiles(a):
        return a[:ty * ts, :tx * ts].reshape(ty, ts, tx, ts).transpose(0, 2, 1, 3).reshape(ty, tx, ts * ts)

    f, g, lm = level0("flat")
    assert len(np.unique(f)) == 1 and not g[0].any() and not g[1].any()
    for s in (0, 1):                                    # an all-zero tile keeps the first pixel of its scan
        assert (lm[s][0] == np.arange(tx)[None, :] * ts).all() and (lm[s][1] == np.arange(ty)[:, None] * ts).all()
    # corner_first / corner_last: every keypoint of both sets at tile offset (0, 0) / (ts - 1, ts - 1); for corner_last the maximum is the
    # tile's only one (a tie would go to an earlier pixel of the scan)
    for kind, o in (("corner_first", 0), ("corner_last", ts - 1)):
        f, g, lm = level0(kind)
        for s in (0, 1):
            assert (lm[s][0] % ts == o).all() and (lm[s][1] % ts == o).all(), (kind, s)
            t = tiles(g[s])
            at_max = (t == t.max(2, keepdims=True)).sum(2)
            inner = at_max[1:, 1:] if kind == "corner_first" else at_max
            assert (inner == 1).all() and (t.max(2) > 0).all(), (kind, s)
    # steps4: more than one pixel at the tile's maximum in at least half of the tiles (in all of them, in fact)
    f, g, lm = level0("steps4")
    assert set(np.unique(f)) == {0, 255} and np.array_equal(f[:, 4:], f[:, :-4]) and np.array_equal(f[4:], f[:-4])
    for s in (0, 1):
        t = tiles(g[s])
        assert ((t == t.max(2, keepdims=True)).sum(2) > 1).mean() >= 0.5
    # rim: the image's first and last row and column hold the extremes
    f, g, lm = level0("rim")
    for edge in (f[0], f[-1], f[:, 0], f[:, -1]):
        assert set(np.unique(edge)) == {0, 255}
    assert f[1:-1, 1:-1].min() >= 64 and f[1:-1, 1:-1].max() < 192
    # remainder: bright pixels only right of and below the last full tile; no keypoint there, yet the last column and row of tiles look at it
    f, g, lm = level0("remainder")
    assert f[:ty * ts, :tx * ts].max() < 8 and f[:, tx * ts:].min() >= 200 and f[ty * ts:].min() >= 200
    for s in (0, 1):
        assert (lm[s][0] < tx * ts).all() and (lm[s][1] < ty * ts).all()
    assert (lm[0][0][:, -1] == tx * ts - 1).all() and (lm[1][1][-1, :] == ty * ts - 1).all()
    with pytest.raises(ValueError):
        S.keyframe_hostile(w, h, "nonsense")


# ---- the comparison can fail ----------------------------------------------------------------------------------------------------------------------
def test_the_comparison_reports_one_wrong_byte_keypoint_or_jacobian_bit():
    w, h = S.KEYFRAME_SIZES[2]
    frames = [S.noise(w, h, 1), S.keyframe_hostile(w, h, "rim", 2), S.noise(w, h, 3), S.keyframe_hostile(w, h, "steps4", 4)]
    want = [S.reference_state(f, O.FMT_GRAY8) for f in frames]
    keys = S.key_frames(4)
    assert keys == [1, 3] and S.call_diffs(copy.deepcopy(want), want, keys) == []

    def damaged(fn):
        got = copy.deepcopy(want)
        fn(got)
        return S.call_diffs(got, want, keys)

    def rim_byte(got):                                  # one rim byte of one level of frame 2
        got[2][1]["img"][-1, -1] ^= 1
    bad = damaged(rim_byte)
    assert len(bad) == 1 and bad[0].startswith("frame 2: level 1: 1 image bytes differ"), bad

    def keypoint(got):                                  # one keypoint of the second keyframe
        got[3][0]["argmax"][1][0, -1, -1] += 1
    bad = damaged(keypoint)
    assert len(bad) == 1 and bad[0].startswith("frame 3: level 0: argmax[1] differs in 1 entries"), bad

    def jac_bit(got):                                   # the last bit of one Jacobian float
        got[1][2]["jac"][0].view(np.uint32)[2, 0, 0] ^= 1
    bad = damaged(jac_bit)
    assert len(bad) == 1 and bad[0].startswith("frame 1: level 2: jac[0] differs in 1 entries"), bad

    def minus_zero(got):                                # -0.0 where 0.0 belongs: equal as floats, not as bits
        assert got[1][0]["jac"][0][3, 0, 0] == 0.0
        got[1][0]["jac"][0][3, 0, 0] = -0.0
    assert len(damaged(minus_zero)) == 1

    def wrong_ts(got):
        got[0][0]["ts"] += 2
    assert damaged(wrong_ts) == ["frame 0: level 0: (w, h, ts) (%d, %d, 8) != (%d, %d, 6)" % (w, h, w, h)]
    # tables of frames that are no keyframes are not part of the state
    def stale_table(got):
        got[2][0]["argmax"][0][:] = 0xA5A5
    assert damaged(stale_table) == []
    assert S.call_diffs(want[:3], want, keys) == ["frames 3 != 4"]
