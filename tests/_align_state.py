"""Helper of tests/test_align_state_cpu.py and tests/test_align_state_gpu.py: the aligner's resident state -- the gray pyramid and the keypoint /
Jacobian tables of every frame of a call -- from the oracle's stage functions, the hostile inputs that go with it, and a numpy restatement of
which route a frame takes through vs_k_ingest_pyr and vs_k_pyr_down_rows.  CPU only: nothing here imports the GPU library or torch."""
import functools

import numpy as np

from oracle import oracle as O

FMT_BITS = {O.FMT_GRAY8: 8, O.FMT_BGR8: 8, O.FMT_BGR10: 10, O.FMT_BGR12: 12, O.FMT_BGR16_FULL: 16}
FMT_OF_BITS = {8: O.FMT_BGR8, 10: O.FMT_BGR10, 12: O.FMT_BGR12, 16: O.FMT_BGR16_FULL}
TINY = dict(pyramid_min_width=4, pyramid_min_height=4)      # pyramids down to a 4-pixel top level


def fmt_dtype(fmt):
    return np.uint8 if FMT_BITS[fmt] == 8 else np.uint16


def fmt_channels(fmt):
    return 1 if fmt == O.FMT_GRAY8 else 3


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def reference_state(frame, fmt, **params):
    """[{w, h, ts, img, argmax[2], jac[2]}] over the pyramid levels of one frame, stage by stage: bgr_to_gray (not for gray input), pyr_down
    again and again, grad_xy -> grad_argmax -> sparse_jac at each level's tile size.  Only the level count and the dimensions come from an
    oracle.Aligner (its first frame does no solve).  Tables as capi.Aligner.keyframe_tables hands them out: (2, ty, tx) u16, (4, ty, tx) f32."""
    frame = np.ascontiguousarray(frame)
    al = O.Aligner(**params)
    al.align_next(frame, fmt=fmt)
    levels = al.debug().levels
    img = frame if fmt == O.FMT_GRAY8 else O.bgr_to_gray(frame, shift_to_8=FMT_BITS[fmt] - 8)
    out = []
    for l in range(levels):
        d = al.level(l)
        assert img.shape == (d["h"], d["w"]), (l, img.shape, d["w"], d["h"])
        ts = O.tile_size(d["w"], d["h"])
        gx, gy = O.grad_xy(img)
        _, lmx, lmy = O.grad_argmax(gx, gy, ts)
        jx, jy = O.sparse_jac(gx, gy, lmx, lmy)
        out.append({"w": d["w"], "h": d["h"], "ts": ts, "img": img, "argmax": [lmx, lmy], "jac": [jx, jy]})
        img = O.pyr_down(img)
    return out


def state_diffs(got, want, tables=True, tag=""):
    """every difference between two states, as text; [] when they are the same bytes.  `tables`: the frame is a keyframe, its keypoint and
    Jacobian tables are part of the state (Jacobians are compared as bit patterns: -0.0 is not 0.0)."""
    bad = []
    if len(got) != len(want):
        return ["%slevels %d != %d" % (tag, len(got), len(want))]
    for l, (g, w) in enumerate(zip(got, want)):
        dims_g, dims_w = tuple(int(g[k]) for k in ("w", "h", "ts")), tuple(int(w[k]) for k in ("w", "h", "ts"))
        if dims_g != dims_w:
            bad.append("%slevel %d: (w, h, ts) %s != %s" % (tag, l, dims_g, dims_w))
            continue
        gi, wi = np.asarray(g["img"]), np.asarray(w["img"])
        if gi.dtype != np.uint8 or gi.shape != wi.shape:
            bad.append("%slevel %d: image %s %s, wanted %s" % (tag, l, gi.dtype, gi.shape, wi.shape))
        elif not np.array_equal(gi, wi):
            ys, xs = np.nonzero(gi != wi)
            bad.append("%slevel %d: %d image bytes differ, first at (x %d, y %d): %d != %d" % (tag, l, ys.size, xs[0], ys[0], gi[ys[0], xs[0]], wi[ys[0], xs[0]]))
        if not tables:
            continue
        for s in (0, 1):
            for name, dt, bits in (("argmax", np.uint16, np.uint16), ("jac", np.float32, np.uint32)):
                ga, wa = np.ascontiguousarray(g[name][s]), np.ascontiguousarray(w[name][s])
                if ga.dtype != dt or ga.shape != wa.shape:
                    bad.append("%slevel %d: %s[%d] %s %s, wanted %s" % (tag, l, name, s, ga.dtype, ga.shape, wa.shape))
                elif not np.array_equal(ga.view(bits), wa.view(bits)):
                    idx = np.argwhere(ga.view(bits) != wa.view(bits))
                    c, ty, tx = idx[0]
                    bad.append("%slevel %d: %s[%d] differs in %d entries, first at (plane %d, tile row %d, tile column %d): %r != %r"
                               % (tag, l, name, s, len(idx), c, ty, tx, ga[c, ty, tx], wa[c, ty, tx]))
    return bad


def key_frames(n, seq0=0, clip_len=0):
    """the frames of an n-frame call that are keyframes: odd index in their sequence (ChunkFrames::g of vs_align_plan.hpp); seq0 = frames
    the handle has seen before the call, clip_len > 0 = a clip call"""
    return [i for i in range(n) if ((i % clip_len) if clip_len else (seq0 + i)) & 1]


def call_diffs(got, want, keyframes):
    """state_diffs over the frames of one call: got / want are lists of states, tables are compared for the frames in `keyframes`"""
    if len(got) != len(want):
        return ["frames %d != %d" % (len(got), len(want))]
    bad = []
    for i, (g, w) in enumerate(zip(got, want)):
        bad += state_diffs(g, w, tables=i in keyframes, tag="frame %d: " % i)
    return bad


def engine_state(aligner, i, tables):
    """frame i of the last call of a capi.Aligner, in reference_state's form (through level() and keyframe_tables(), that is,
    vs_aligner_level_dims and vs_aligner_read_level_image / _argmax / _jacobian)"""
    out = []
    for l in range(aligner.info(i).levels):
        d = aligner.level(i, l)
        e = {"w": d["w"], "h": d["h"], "ts": d["ts"], "img": d["img"]}
        if tables:
            e.update(aligner.keyframe_tables(i, l))
        out.append(e)
    return out


# ---- the gray formula at its rounding boundary -------------------------------------------------------------------------------------------
WB, WG, WR = 3735, 19235, 9798                       # the 15-bit weights of cv::cvtColor(BGR2GRAY); their sum is 32768


def gray_numpy(bgr, bits, rounding=16384, weights=(WB, WG, WR)):
    """the gray formula on an (n, 3) array of colours, in 64-bit integers"""
    c = np.asarray(bgr, np.int64)
    v = (c[:, 0] * weights[0] + c[:, 1] * weights[1] + c[:, 2] * weights[2] + rounding) >> 15
    return np.minimum(v >> (bits - 8), 255)


def gray_split_numpy(bgr, lowered=None):
    """the u8 group route's form: byte 2 of B*b + G*g + R*r + 32768 with each doubled weight split as (w >> 7) * 256 + 2 * (w & 127);
    `lowered`: the channel whose split weight is one too small"""
    c = np.asarray(bgr, np.int64)
    ws = [(w >> 7) * 256 + 2 * (w & 127) - (1 if lowered == k else 0) for k, w in enumerate((WB, WG, WR))]
    return ((c[:, 0] * ws[0] + c[:, 1] * ws[1] + c[:, 2] * ws[2] + 32768) >> 16) & 255


def residue(bgr, bits):
    """(S + 16384) mod the step of the gray value, 32768 << (bits - 8): 0 = the gray has just stepped up, step - 1 = about to step"""
    c = np.asarray(bgr, np.int64)
    return (c[:, 0] * WB + c[:, 1] * WG + c[:, 2] * WR + 16384) % (32768 << (bits - 8))


PALETTE_KEEP = 1500                                  # colours kept per side where the candidates are many


def _nearest(cols, res, keep):
    order = np.argsort(res, kind="stable")
    return cols[order[:keep]]


@functools.lru_cache(maxsize=None)
def _palette_sides(bits):
    step, hi = 32768 << (bits - 8), (1 << bits) - 1
    if bits == 8:
        # every one of the 2^24 colours: all of those with residue 0 and all of those with the largest residue there is
        b, g = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
        base = (b * WB + g * WG + 16384).ravel()
        res = np.stack([(base + r * WR) % step for r in range(256)], 1)          # [b * 256 + g, r]
        top = int(res.max())

        def cols_at(value):
            i, r = np.nonzero(res == value)
            return np.stack([i // 256, i % 256, r], 1)
        return cols_at(0), cols_at(top)
    if bits == 10:
        # the residue depends on (B - R, G - R) and, for a step of 4 * 32768, on R mod 4: every pair, every R mod 4 it allows
        d = np.arange(-hi, hi + 1, dtype=np.int64)
        db, dg = (a.ravel() for a in np.meshgrid(d, d, indexing="ij"))
        lo, top = np.maximum(0, np.maximum(-db, -dg)), np.minimum(hi, np.minimum(hi - db, hi - dg))
        cols, ress = [], []
        for r4 in range(4):
            r = lo + ((r4 - lo) % 4)
            ok = r <= top
            c = np.stack([r + db, r + dg, r], 1)[ok]
            cols.append(c)
            ress.append(residue(c, bits))
        cols, ress = np.concatenate(cols), np.concatenate(ress)
        return _nearest(cols, ress, PALETTE_KEEP), _nearest(cols, step - 1 - ress, PALETTE_KEEP)
    # 12 and 16 bits: seeded draws.  A colour drawn whole lands within a few units of the boundary at best (one in `step` lands on it), so
    # B and G are drawn, four million pairs, and R is the channel value that puts the colour at the wanted distance from the boundary --
    # where one exists inside the format: 9798 R = target - (3735 B + 19235 G + 16384) mod step, 9798 = 2 * 4899, 4899 odd.
    rng = np.random.default_rng(1000 + bits)
    n = 4_000_000
    b, g = rng.integers(0, hi + 1, n, dtype=np.int64), rng.integers(0, hi + 1, n, dtype=np.int64)
    inv = pow(WR // 2, -1, step // 2)
    sides = []
    for targets in ((0, 1, 2), (step - 1, step - 2, step - 3)):
        found = []
        for t in targets:
            rhs = (t - (b * WB + g * WG + 16384)) % step
            r = ((rhs // 2) * inv) % (step // 2)
            ok = (rhs % 2 == 0) & (r <= hi)
            found.append(np.stack([b, g, r], 1)[ok][:PALETTE_KEEP // 3])
        sides.append(np.concatenate(found))
    return sides[0], sides[1]


def boundary_palette(bits):
    """{"above", "below", "corners", "over"}: (n, 3) int64 BGR colours of a `bits`-deep format.  above / below: the colours whose exact sum
    S + 16384 lies nearest to a multiple of 32768 << (bits - 8), having just passed it (residue 0, 1, ..) or about to (step - 1, ..).
    corners: all 0, all max, each channel alone at max.  over (u16 containers below 16 bits): values above the format's maximum."""
    above, below = _palette_sides(bits)
    hi = (1 << bits) - 1
    corners = np.array([[0, 0, 0], [hi, hi, hi], [hi, 0, 0], [0, hi, 0], [0, 0, hi]], np.int64)
    over = np.zeros((0, 3), np.int64)
    if 8 < bits < 16:
        m = 0xFFFF
        over = np.array([[m, m, m], [m, 0, 0], [0, m, 0], [0, 0, m], [hi + 1, hi + 1, hi + 1], [hi + 1, hi, hi], [hi, hi, hi + 1],
                         [m, hi, 0], [0, m, hi], [2 * hi + 1, 0, 3], [hi, 2 * hi, hi]], np.int64)
    return {"above": above, "below": below, "corners": corners, "over": over}


def palette_colours(bits):
    p = boundary_palette(bits)
    return np.concatenate([p["above"], p["below"], p["corners"], p["over"]])


def palette_frame(w, h, bits, seed):
    """(h, w, 3) frame whose pixels are drawn from boundary_palette(bits) in random order (every colour appears while there is room)"""
    cols = palette_colours(bits)
    rng = np.random.default_rng(seed)
    n = w * h
    pick = np.concatenate([rng.permutation(len(cols))] * (n // len(cols)) + [rng.permutation(len(cols))[:n % len(cols)]])
    pick = pick[rng.permutation(n)]
    return cols[pick].reshape(h, w, 3).astype(np.uint8 if bits == 8 else np.uint16)


# ---- hostile gray keyframes -----------------------------------------------------------------------------------------------------------------
KINDS = ("flat", "steps4", "corner_first", "corner_last", "rim", "remainder")


def noise(w, h, seed, fmt=O.FMT_GRAY8):
    rng = np.random.default_rng(seed)
    shape = (h, w) if fmt == O.FMT_GRAY8 else (h, w, 3)
    return rng.integers(0, 1 << FMT_BITS[fmt], shape).astype(fmt_dtype(fmt))


def keyframe_hostile(w, h, kind, seed=0):
    """gray u8 frames against the keyframe kernel; ts = the level-0 tile size"""
    ts = O.tile_size(w, h)
    tx, ty = w // ts, h // ts
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return noise(w, h, seed)
    if kind == "flat":
        return np.full((h, w), int(rng.integers(0, 256)), np.uint8)
    if kind == "steps4":
        # 0 / 255 steps of period 4 along x and along y: thousands of pixels tie at the largest gradient, the smallest scan index wins
        y, x = np.mgrid[0:h, 0:w]
        return np.where(((x // 2) + (y // 2)) % 2 == 0, 0, 255).astype(np.uint8)
    if kind in ("corner_first", "corner_last"):
        # The one gradient maximum of every tile, in x and in y, at tile offset (o, o): o = 0 or ts - 1.  A single bright pixel cannot do
        # that -- a central difference answers an impulse, and a step, at TWO pixels -- so the frame is mid-gray with a staircase along
        # every row y = o (mod ts) and along every column x = o (mod ts): plateaus of 1 and 255 that change at the target pixels, which
        # hold 128 themselves.  At a target the neighbours differ by 254 (|g| = 127); one pixel further, and everywhere else, by 127 at
        # most.  (The targets in column 0 / row 0 of corner_first see a clamped neighbour: 63.5, a tie with pixels that follow them in
        # the scan.)  For o = ts - 1 the right neighbour of the last tile's target lies in the remainder strip and the lower neighbour
        # of a tile's last row is row `ts` of its walk.
        o = 0 if kind == "corner_first" else ts - 1
        assert kind == "corner_first" or (w % ts and h % ts), "corner_last needs w %% ts and h %% ts non-zero (%d x %d, ts %d)" % (w, h, ts)

        def stairs(n):
            d = np.arange(n) - o
            return np.where(d % ts == 0, 128, np.where((d // ts + 1) % 2 == 1, 255, 1)).astype(np.uint8)
        img = np.full((h, w), 128, np.uint8)
        img[o::ts, :] = stairs(w)[None, :]
        img[:, o::ts] = stairs(h)[:, None]
        return img
    if kind == "rim":
        img = rng.integers(64, 192, (h, w)).astype(np.uint8)
        ext = np.array([0, 255], np.uint8)
        img[0, :], img[h - 1, :] = ext[rng.integers(0, 2, w)], ext[rng.integers(0, 2, w)]
        img[:, 0], img[:, w - 1] = ext[rng.integers(0, 2, h)], ext[rng.integers(0, 2, h)]
        return img
    if kind == "remainder":
        assert w % ts and h % ts, "the remainder strip needs w %% ts and h %% ts non-zero (%d x %d, ts %d)" % (w, h, ts)
        img = np.full((h, w), 3, np.uint8)
        img[:, tx * ts:] = rng.integers(200, 256, (h, w - tx * ts))
        img[ty * ts:, :] = rng.integers(200, 256, (h - ty * ts, w))
        return img
    raise ValueError(kind)


# ---- frames inside a larger buffer ------------------------------------------------------------------------------------------------------------
TAIL = 64                                           # filled elements behind the last row


def embed(frames, pitch, frame_pitch, base_off, fill):
    """frames (n, h, w[, 3]) -> (flat buffer full of `fill` but for the frames, element offset of frame 0).  Row r of frame i starts at
    element base_off + i * frame_pitch + r * pitch."""
    frames = np.asarray(frames)
    n, h = frames.shape[:2]
    rows = frames.reshape(n, h, -1)
    row_len = rows.shape[2]
    assert pitch >= row_len and (n == 1 or frame_pitch >= (h - 1) * pitch + row_len)
    buf = np.full(base_off + (n - 1) * frame_pitch + (h - 1) * pitch + row_len + TAIL, fill, frames.dtype)
    es = frames.dtype.itemsize
    view = np.lib.stride_tricks.as_strided(buf[base_off:], (n, h, row_len), (frame_pitch * es, pitch * es, es))
    view[:] = rows
    return buf, base_off


# ---- which way a frame goes ----------------------------------------------------------------------------------------------------------------------
class Route(tuple):
    """(kind, interior, one_column, w % 4): kind "byte" or "group"; interior: some tile of the group route takes the interior build;
    one_column: tiles_x == 1"""
    __slots__ = ()
    kind = property(lambda s: s[0])
    interior = property(lambda s: s[1])
    one_column = property(lambda s: s[2])
    wmod4 = property(lambda s: s[3])


def ingest_route(w, h, elem_bytes, pitch, base_byte_off, frame_pitch, i):
    """the route of frame i through vs_k_ingest_pyr: pitches in elements, base_byte_off = the address of frame 0 modulo 4 (0 for host
    frames: they are copied to the start of a device allocation)"""
    tiles_x, tiles_y = -(-w // 128), -(-h // 32)
    aligned = (base_byte_off + i * frame_pitch * elem_bytes) % 4 == 0 and (pitch * elem_bytes) % 4 == 0
    if not aligned or w < 4:
        return Route(("byte", False, tiles_x == 1, w % 4))
    interior = False
    if w % 4 == 0:
        for tyi in range(tiles_y):
            for txi in range(tiles_x):
                ix0, iy0 = 2 * (64 * txi) - 4, 2 * (16 * tyi) - 2
                interior |= ix0 >= 0 and ix0 + 136 <= w and iy0 >= 0 and iy0 + 35 <= h
    return Route(("group", interior, tiles_x == 1, w % 4))


def pyr_route(n_frames_in_call):
    """rows per band of vs_k_pyr_down_rows as vsk::pyr_down picks them"""
    return 4 if n_frames_in_call <= 4 else 16


# ---- the tables of section 3 -------------------------------------------------------------------------------------------------------------------------
# every frame of a batch: (w, h), all with pyramids down to 4 pixels (TINY)
BATCH_SIZES = [
    (499, 131),     # w % 4 = 3; level 1 is 249 wide: one column past the 248-column strip; level heights 65 = 16k + 1, 32, 16
    (496, 134),     # w % 4 = 0, interior ingest tiles; level 1 is 248 wide: exactly one strip; level 2 is 33 high = 16k + 1
    (494, 99),      # w % 4 = 2; level 1 is 247 wide: one column short of the strip
    (129, 33),      # the 128 x 32 ingest tile + 1: a second tile column and row of one pixel; w % 4 = 1
    (128, 32),      # the ingest tile itself: tiles_x == 1
    (127, 31),      # the ingest tile - 1, w <= 128
    (150, 130),     # top level 4 x 4: every word of its rows clamps to w - 4
    (203, 170),     # top level 6 x 5
]
BATCH_FORMATS = [O.FMT_BGR8, O.FMT_BGR10, O.FMT_GRAY8]
# (name, n_clips, frames per call ...): batches on one handle, or one clip call
BATCH_CALLS = [("batch1", 0, (1,)), ("batch3", 0, (3,)), ("batch6", 0, (6,)), ("batch3then4", 0, (3, 4)), ("clips3", 2, (6,)), ("clips4", 2, (8,))]

# routes of the ingest: (format, w, h, frames, pitch, frame_pitch, base_off); pitches and the offset in elements, None = dense
_8, _10 = O.FMT_BGR8, O.FMT_BGR10
ROUTE_CASES = [
    (_8, 131, 67, 2, None, None, 0),              # dense, odd width: pitch 393 -> byte loop
    (_8, 132, 67, 2, None, None, 0),              # group route, rim tiles only
    (_8, 132, 67, 2, 398, None, 0),               # w % 4 == 0 on a pitch that is no multiple of 4 -> byte loop
    (_8, 264, 70, 2, None, None, 0),              # group route with an interior tile
    (_8, 264, 70, 2, 264 * 3 + 12, None, 0),      # ... on a padded pitch
    (_8, 128, 40, 2, None, None, 0),              # tiles_x == 1
    (_8, 133, 67, 2, 400, None, 0),               # group route at w % 4 = 1: the right-rim group starts at byte 387 of its row
    (_8, 134, 67, 2, 404, None, 0),               # w % 4 = 2
    (_8, 135, 67, 2, 408, None, 0),               # w % 4 = 3
    (_8, 479, 71, 2, 1452, None, 0),              # w % 4 = 3, three tile columns and rows
    (_8, 132, 67, 2, None, None, 1),              # base offsets: byte loop for device frames
    (_8, 135, 67, 2, 408, None, 2),
    (_8, 264, 70, 2, None, None, 3),
    (_8, 132, 67, 3, None, 67 * 396 + 2, 0),      # frame 0 aligned, frame 1 not, frame 2 again: the route changes inside one launch
    (_8, 133, 67, 3, 400, 67 * 400 + 1, 0),
    (_10, 131, 67, 2, None, None, 0),             # dense, odd width: odd pitch -> byte loop
    (_10, 132, 67, 2, None, None, 0),             # group route, rim tiles only
    (_10, 264, 70, 2, None, None, 0),             # interior tile
    (_10, 264, 70, 2, 264 * 3 + 6, None, 0),
    (_10, 128, 40, 2, None, None, 0),             # tiles_x == 1
    (_10, 133, 67, 2, 400, None, 0),              # odd width on an even pitch: group route at w % 4 = 1
    (_10, 134, 67, 2, None, None, 0),             # w % 4 = 2 (dense: pitch 402 is even)
    (_10, 135, 67, 2, 406, None, 0),              # w % 4 = 3
    (_10, 132, 67, 2, None, None, 1),             # base offsets: 2 bytes -> byte loop, 4 bytes -> group route, 6 bytes -> byte loop
    (_10, 133, 67, 2, 400, None, 2),
    (_10, 264, 70, 2, None, None, 3),
    (_10, 132, 67, 3, None, 67 * 396 + 1, 0),     # frame 1 two bytes off
    (_10, 135, 67, 3, 406, 67 * 406 + 3, 0),
]


def route_case_layout(case):
    """(pitch, frame_pitch, base_off) of a route case with the dense defaults filled in"""
    fmt, w, h, n, pitch, frame_pitch, base_off = case
    pitch = pitch or w * 3
    return pitch, frame_pitch or h * pitch, base_off


def route_case_routes(case, device):
    fmt, w, h, n = case[:4]
    pitch, frame_pitch, base_off = route_case_layout(case)
    es = np.dtype(fmt_dtype(fmt)).itemsize
    return [ingest_route(w, h, es, pitch, (base_off * es) % 4 if device else 0, frame_pitch, i) for i in range(n)]


# formats and boundary colours: (bits, w, h, pitch); None = dense.  264 x 70 has interior tiles, 133 x 67 has none; dense and padded so that
# each size meets the palette on the group route and in the byte loop
def palette_cases():
    cases = []
    for bits in (8, 10, 12, 16):
        cases += [(bits, 264, 70, None), (bits, 264, 70, 264 * 3 + (2 if bits == 8 else 1)), (bits, 133, 67, None), (bits, 133, 67, 400)]
    return cases


# keyframe tables at every tile size: gray (w, h) whose level-0 tile size runs through 2, 4, .., 20; w % ts and h % ts non-zero everywhere
KEYFRAME_SIZES = [(127, 121), (139, 133), (203, 191), (269, 253), (335, 327), (401, 389), (467, 453), (533, 517), (599, 581), (663, 645)]
# kinds of the two keyframes (frames 1 and 3) of each 4-frame call
KEYFRAME_CALLS = [("noise", "flat"), ("steps4", "corner_first"), ("corner_last", "rim"), ("remainder", "noise"), ("flat", "steps4")]


def tiles_per_wave(ts):
    """keyframe_rows_tiles_per_wave of vs_kernels.hip"""
    return 62 // (ts // (4 if ts % 4 == 0 else 2))


def level_dims(w, h, **params):
    """[(w, h, ts)] over the levels, as build_levels / ComputePyramid count them"""
    p = dict(pyramid_min_width=20, pyramid_min_height=20)
    p.update(params)
    lv, ww, hh = 0, w, h
    while True:
        lv, ww, hh = lv + 1, ww // 2, hh // 2
        if not (ww >= p["pyramid_min_width"] and hh >= p["pyramid_min_height"]):
            break
    return [(w >> l, h >> l, O.tile_size(w >> l, h >> l)) for l in range(lv)]
