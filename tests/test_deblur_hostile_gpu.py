"""The deblur kernels (vs_deblur.hip) where the first tests never went: rint ties, tile and group seams, frames smaller than a wave, NaN /
infinite / singular maps, samples above the format's maximum, ratio edges, the parameter boundary -- bit for bit against the rule's
restatement (tests/_deblur_ref.py), and within the fp32 error bound of the rule written directly in float64 (tests/_deblur_direct.py).
Inputs and their premises: tests/_hostile_maps.py; every premise is asserted on the CPU references before a kernel runs.

Every kernel-level call here works on DEVICE memory (torch tensors) with the destination inside a guard band on all four sides: the
host-memory form of the call copies only the rows' own bytes back, so a guard band round a host buffer proves nothing about the kernel."""
import ctypes as C

import numpy as np
import pytest

import _deblur_direct as D
import _deblur_ref as R
import _hostile_maps as HM

pytestmark = pytest.mark.gpu

FORMATS = HM.FORMATS
G = 3                                                                # guard rows above and below every destination frame


def _ref_batch(vs, src, S, cf, ct, bits, maxv, sens=2.0, max_ratio=4.0):
    with np.errstate(all="ignore"):                                  # (NaN and infinite maps: the comparisons are false, as in the kernels)
        return R.deblur_batch(HM.cvinv(vs), src, S, cf, ct, bits, maxv, sens, max_ratio)


def _dev_call(vs, src, S, cf, ct, fmt, params=None, ss=None, ds=None, src_gap=0, src_off=0, dst_off=0):
    """vs_bgr_deblur_batch on device memory.  ss / ds: row strides (elements); src_gap: elements between the source frames; src_off /
    dst_off: elements in front of the first frame (alignment).  The destination frames lie G rows apart inside a buffer filled with a guard
    value: everything but the frames' own samples must come back untouched.  -> (n_out, h, w, 3)"""
    import torch
    src = np.ascontiguousarray(src)
    n_src, h, w, _ = src.shape
    dtype, esz = src.dtype, src.dtype.itemsize
    ss = 3 * w if ss is None else ss
    ds = 3 * w if ds is None else ds
    sfs = h * ss + src_gap
    host = np.zeros(src_off + n_src * sfs + 8, dtype)
    for i in range(n_src):
        host[src_off + i * sfs:src_off + i * sfs + h * ss].reshape(h, ss)[:, :3 * w] = src[i].reshape(h, 3 * w)
    idx = np.ascontiguousarray(cf, np.int32)
    n_out, n_cand = idx.shape
    flat = [t for row in ct for t in row]
    assert len(flat) == n_out * n_cand
    arr = (vs.Transform * len(flat))(*flat)
    dfs = (h + 2 * G) * ds
    guard = 0x5A if esz == 1 else 0x5A5A
    dhost = np.full(dst_off + n_out * dfs + 8, guard, dtype)
    as_t = (lambda a: torch.from_numpy(a.view(np.int16) if esz == 2 else a).cuda())
    dsrc, ddst = as_t(host), as_t(dhost)
    dS = torch.from_numpy(np.ascontiguousarray(S, np.uint64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    vs._check(vs.lib().vs_bgr_deblur_batch(C.c_void_p(dsrc.data_ptr() + src_off * esz), sfs, n_src, w, h, ss, fmt, C.c_void_p(dS.data_ptr()), n_out, n_cand,
                                           idx.ctypes.data_as(C.POINTER(C.c_int32)), arr, C.byref(params) if params is not None else None,
                                           C.c_void_p(ddst.data_ptr() + (dst_off + G * ds) * esz), dfs, ds, vs.MEM_DEVICE, None))
    torch.cuda.synchronize()
    back = ddst.cpu().numpy().view(dtype).copy()
    frames = back[dst_off:dst_off + n_out * dfs].reshape(n_out, h + 2 * G, ds)
    res = frames[:, G:G + h, :3 * w].reshape(n_out, h, w, 3).copy()
    frames[:, G:G + h, :3 * w] = guard
    assert (frames[:, :G] == guard).all(), "rows above a destination frame were written"
    assert (frames[:, G + h:] == guard).all(), "rows below a destination frame were written"
    assert (frames[:, G:G + h, 3 * w:] == guard).all(), "the tail of a destination row was written"
    assert (back == guard).all(), "memory in front of or behind the destination was written"
    return res


def _dword_stride(w, esz, extra=0):
    s = 3 * w + extra
    while (s * esz) % 4:
        s += 1
    return s


@pytest.mark.parametrize("shape", HM.DEBLUR_SHAPES, ids=["%dx%d" % s for s in HM.DEBLUR_SHAPES])
def test_shapes_seams_ties_and_hostile_maps_equal_the_rule(gpu_vs, shape):
    """every format at one shape: tiny and one-sided frames, frames across the per-sample kernel's 64 x 64 tile and the x4 kernel's
    256 x 64 tile; candidates with tie maps, rotations to 0.5 rad, NaN / singular / near-singular / quarter-turn maps (HM.deblur_case)"""
    vs = gpu_vs
    w, h = shape
    for fmt in sorted(FORMATS):
        code, dtype, bits = FORMATS[fmt]
        maxv = (1 << bits) - 1
        esz = np.dtype(dtype).itemsize
        src, S, cf, maps = HM.deblur_case(vs, fmt, w, h)
        ct = HM.transforms(vs, maps)
        want = _ref_batch(vs, src, S, cf, ct, bits, maxv)
        assert np.array_equal(want[2], src[5])                      # the sharpest frame: a copy
        if w >= 4 and h >= 4:
            assert (want != src[cf[:, 0]]).mean() > 0.05            # the candidates change the frames: the case has teeth
        got = _dev_call(vs, src, S, cf, ct, code)
        assert np.array_equal(got, want), (fmt, "dense", int((got != want).sum()))
        got = _dev_call(vs, src, S, cf, ct, code, ss=3 * w + 7, ds=3 * w + 5)
        assert np.array_equal(got, want), (fmt, "pitched", int((got != want).sum()))
        got = _dev_call(vs, src, S, cf, ct, code, ss=_dword_stride(w, esz, 5), ds=_dword_stride(w, esz, 2))
        assert np.array_equal(got, want), (fmt, "pitched on dwords", int((got != want).sum()))


@pytest.mark.parametrize("shape", [(64, 16), (260, 65)], ids=["64x16", "260x65"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr10"])
def test_a_group_with_one_unaligned_target_or_destination_gives_the_aligned_run_s_frames(gpu_vs, fmt, shape):
    """widths that are multiples of 4, so that the dense run takes the x4 kernel; then a frame stride, a first frame, a destination stride and
    a destination that do not start on a dword: the whole group falls back to the per-sample kernel and the frames are the same"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    esz = np.dtype(dtype).itemsize
    w, h = shape
    src, S, cf, maps = HM.deblur_case(vs, fmt, w, h)
    ct = HM.transforms(vs, maps)
    want = _ref_batch(vs, src, S, cf, ct, bits, maxv)
    aligned = _dev_call(vs, src, S, cf, ct, code)
    assert np.array_equal(aligned, want)
    gap = 1 if esz == 2 else 3                                       # the frame stride: rows on dwords, every other frame (16-bit) or three of four (8-bit) off them
    assert w % 4 == 0 and (3 * w * esz) % 4 == 0 and ((h * 3 * w + gap) * esz) % 4 != 0
    for kw in (dict(src_gap=gap), dict(src_off=1), dict(ds=3 * w + 1), dict(dst_off=1), dict(src_gap=gap, ds=3 * w + 1, dst_off=1)):
        got = _dev_call(vs, src, S, cf, ct, code, **kw)
        assert np.array_equal(got, aligned), (kw, int((got != aligned).sum()))


@pytest.mark.parametrize("shape", [(64, 48), (63, 47), (260, 75)], ids=["64x48", "63x47", "260x75"])
def test_ties_round_to_even(gpu_vs, shape, monkeypatch):
    """every pixel of the last candidate lies on a tie (half-integer translations in x, in y, in both, the positions -0.5, w - 1.5 and
    w - 0.5 among them; a rotated map of exact entries), with 2 and with 16 candidates.  Premise: a restatement that rounds half up differs
    from the rule's at more than a tenth of the samples"""
    vs = gpu_vs
    w, h = shape
    ties = HM.tie_maps(vs, w, h)
    for fmt in ("bgr8", "bgr10"):
        code, dtype, bits = FORMATS[fmt]
        maxv = (1 << bits) - 1
        rng = np.random.default_rng(w + bits)
        src = HM.contrast_stack(rng, 6, w, h, dtype, maxv)
        S = R.sharpness_batch(src, bits)
        assert all(S[i] < S[i + 1] for i in range(5))
        for n_cand in (2, 16):
            cf = np.array([[o % 3] + [3 + (c % 3) for c in range(n_cand - 1)] for o in range(len(ties))], np.int32)
            maps = [[(0.0, 0.0, 0.0, 0.0)] + [HM._rot(rng, w, h, big=c % 2 == 0) for c in range(n_cand - 2)] + [tr] for _, tr in ties]
            ct = HM.transforms(vs, maps)
            want = _ref_batch(vs, src, S, cf, ct, bits, maxv)
            with monkeypatch.context() as m:
                def half_up(M, w_, h_):
                    M = np.asarray(M, np.float64).reshape(6)
                    xs, ys = np.arange(w_, dtype=np.float64)[None, :], np.arange(h_, dtype=np.float64)[:, None]
                    return np.floor((M[0] * xs + M[1] * ys) + M[2] + 0.5), np.floor((M[3] * xs + M[4] * ys) + M[5] + 0.5)
                m.setattr(R, "nearest_map", half_up)
                wrong = _ref_batch(vs, src, S, cf, ct, bits, maxv)
            assert (wrong != want).mean() > 0.1, (fmt, n_cand, float((wrong != want).mean()))
            got = _dev_call(vs, src, S, cf, ct, code)
            assert np.array_equal(got, want), (fmt, n_cand, int((got != want).sum()), int((got != wrong).sum()))


@pytest.mark.parametrize("shape", [(64, 16), (67, 20)], ids=["64x16_x4", "67x20"])
@pytest.mark.parametrize("fmt", ["bgr8", "bgr16"])
def test_hostile_maps_contribute_what_the_rule_says(gpu_vs, fmt, shape):
    """NaN in each field, infinite and 1e300 shifts, the singular and the near-singular transforms, quarter and half turns with zoom 0.5 and
    2, each as candidate 1 in front of an ordinary candidate 2.  A map with a NaN or a shift out of every frame contributes nothing: the
    result is the frame deblurred from candidate 2 alone.  The singular map contributes candidate pixel (0, 0) everywhere"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = shape
    rng = np.random.default_rng(7 * w + bits)
    src = HM.contrast_stack(rng, 6, w, h, dtype, maxv)
    S = HM.SYNTH_S
    names = sorted(HM.HOSTILE)
    ordinary = HM._rot(rng, w, h)
    cf = np.array([[0, 5, 4]] * len(names), np.int32)
    maps = [[(0.0, 0.0, 0.0, 0.0), HM.HOSTILE[n], ordinary] for n in names]
    ct = HM.transforms(vs, maps)
    want = _ref_batch(vs, src, S, cf, ct, bits, maxv)
    alone = _ref_batch(vs, src, S, [[0, 4]], HM.transforms(vs, [[maps[0][0], ordinary]]), bits, maxv)[0]
    for i, n in enumerate(names):
        M = np.asarray(HM.cvinv(vs)(ct[i][1], w, h), np.float64)
        if n in HM.HAS_NAN:
            assert np.isnan(M).any(), n
        if n in HM.HAS_NAN or "1e300" in n:
            assert np.array_equal(want[i], alone), n
        if n == "singular":
            assert not M.any()
            with np.errstate(all="ignore"):
                _, W = R.deblur_frame(HM.cvinv(vs), src, S, [0, 5], ct[i][:2], bits, maxv, want_weight=True)
            assert (W > 1).all() and not np.array_equal(want[i], alone)
    got = _dev_call(vs, src, S, cf, ct, code)
    for i, n in enumerate(names):
        assert np.array_equal(got[i], want[i]), (n, int((got[i] != want[i]).sum()))
    got = _dev_call(vs, src, S, cf, ct, code, ss=3 * w + 7, ds=3 * w + 5)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", [(63, 15), (64, 16), (260, 65)], ids=["63x15", "64x16_x4", "260x65_x4"])
@pytest.mark.parametrize("fmt", ["bgr10", "bgr12"])
def test_samples_above_the_format_s_maximum(gpu_vs, fmt, shape):
    """containers that hold 65535 and max_value + 1 at scattered pixels of targets and candidates: the gray's min(g, 255) and the output's
    saturation are both live (premises, on the restatement)"""
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    w, h = shape
    rng = np.random.default_rng(w * bits)
    src = HM.out_of_range_stack(rng, 6, w, h, bits)
    want_S = R.sharpness_batch(src, bits)
    g = R.gray_unclamped(src, bits)
    unclamped = ((g[:, 1:-1, 2:] - g[:, 1:-1, :-2]) ** 2 + (g[:, 2:, 1:-1] - g[:, :-2, 1:-1]) ** 2).sum(axis=(1, 2))
    assert (unclamped.astype(np.uint64) != want_S).all()             # without the gray's clamp every frame's S would be another
    assert np.array_equal(vs.sharpness_batch(src, fmt=code), want_S)
    assert np.array_equal(vs.sharpness_batch(src, fmt=code, src_stride=3 * w + 7), want_S)          # (the per-sample kernel whatever the width)
    _, _, cf, maps = HM.deblur_case(vs, fmt, w, h)
    ct = HM.transforms(vs, maps)
    S = HM.SYNTH_S
    want = _ref_batch(vs, src, S, cf, ct, bits, maxv)
    live = False
    for o in range(len(cf)):
        with np.errstate(all="ignore"):
            _, _, raw = R.deblur_frame(HM.cvinv(vs), src, S, list(cf[o]), ct[o], bits, maxv, want_raw=True)
        live |= bool((raw > maxv).any())
    assert live, "the unclamped blend never exceeds max_value: the input has to change"
    got = _dev_call(vs, src, S, cf, ct, code)
    assert np.array_equal(got, want), int((got != want).sum())
    assert got[[0, 1, 3]].max() == maxv and got[2].max() == 65535    # a blended frame is saturated; a copied one comes back bit for bit
    got = _dev_call(vs, src, S, cf, ct, code, ss=3 * w + 7, ds=3 * w + 5)
    assert np.array_equal(got, want)


def _edge_frames():
    """16 x 12 8-bit frames whose sharpness is known: black (0); one rim pixel raised by one gray step next to black interior pixels (1); a
    noise patch (S2) and the same with the rim pixel (S2 + 1); an interior bump of 1 (4) and of 3 (36)"""
    w, h = 16, 12
    f = np.zeros((6, h, w, 3), np.uint8)
    f[1, 3, 0] = (8, 0, 0)                                           # (8 * 3735 + 16384) >> 15 = 1: one gray step, a sample a blend can show
    f[2, 2:10, 6:14] = np.random.default_rng(5).integers(0, 256, (8, 8, 3))
    f[3] = f[2]
    f[3, 3, 0] = (8, 0, 0)
    f[4, 6, 8] = 1
    f[5, 6, 8] = 3
    return f


def test_ratio_edges(gpu_vs):
    vs = gpu_vs
    src = _edge_frames()
    S = R.sharpness_batch(src, 8)
    assert np.array_equal(vs.sharpness_batch(src), S)
    assert S[0] == 0 and S[1] == 1 and S[3] == S[2] + 1 and S[2] > 1000 and S[4] == 4 and S[5] == 36
    ident = vs.Transform.of()
    shift = vs.Transform.of(0.0, 0.0, 1.0, 0.0)
    # S_k = 0 with S_j = 1; S_k = 1; S_j = S_k + 1; S_j = S_k - 1 (a copy); the only sharper candidate behind a -1 (a copy); ratio 9
    cf = np.array([[0, 1, -1], [1, 4, 5], [2, 3, -1], [3, 2, -1], [2, -1, 3], [4, 5, -1]], np.int32)
    ct = [[ident, shift, ident]] * len(cf)
    for mr in (4.0, 9.0, float(np.nextafter(np.float32(9.0), np.float32(0))), float(np.nextafter(np.float32(9.0), np.float32(99))), 1.0, 36.0):
        p = vs.deblur_params(sensitivity=0.5, max_ratio=mr)
        want = _ref_batch(vs, src, S, cf, ct, 8, 255, 0.5, mr)
        assert np.array_equal(want[3], src[3]) and np.array_equal(want[4], src[2])
        assert not np.array_equal(want[0], src[0]) and not np.array_equal(want[2], src[2]) and not np.array_equal(want[5], src[4])
        got = _dev_call(vs, src, S, cf, ct, vs.FMT_BGR8, params=p)
        assert np.array_equal(got, want), (mr, int((got != want).sum()))
    # the ratio sits at max_ratio exactly: one ulp below it the weight is smaller and the restatement's W shows it
    _, Wa = R.deblur_frame(HM.cvinv(vs), src, S, [4, 5], [ident, ident], 8, 255, 0.5, 9.0, want_weight=True)
    _, Wb = R.deblur_frame(HM.cvinv(vs), src, S, [4, 5], [ident, ident], 8, 255, 0.5, float(np.nextafter(np.float32(9.0), np.float32(0))), want_weight=True)
    _, Wc = R.deblur_frame(HM.cvinv(vs), src, S, [4, 5], [ident, ident], 8, 255, 0.5, float(np.nextafter(np.float32(9.0), np.float32(99))), want_weight=True)
    assert (Wb < Wa).all() and np.array_equal(Wa, Wc)


def test_parameter_boundary(gpu_vs):
    """include/vs_amd.h's condition on vs_deblur_params: just inside it the black target under the largest ratios equals the restatement,
    whose W is finite; just outside it the call and the stabilizer refuse with VS_ERR_ARG"""
    vs = gpu_vs
    src, _ = HM.black_target_stack(np.random.default_rng(3))
    S = HM.BIG_S
    cf, ct = np.array([[0, 1, 2]], np.int32), [[vs.Transform.of()] * 3]
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))
    above = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    for sens, mr in ((2.0 ** -96, 4.0), (1.0, 2.0 ** 50), (2.0 ** 6, 1.0e18), (2.0, 4.0), (0.5, 1.75), (8.0, 100.0)):
        assert HM.params_accepted(sens, mr)
        with np.errstate(all="raise"):
            out, W, raw = R.deblur_frame(HM.cvinv(vs), src, S, [0, 1, 2], ct[0], 16, 65535, sens, mr, want_raw=True)
        assert np.isfinite(W).all() and np.isfinite(raw).all()
        p = vs.deblur_params(sensitivity=sens, max_ratio=mr)
        got = _dev_call(vs, src, S, cf, ct, vs.FMT_BGR16_FULL, params=p)
        assert np.array_equal(got[0], out), (sens, mr, int((got[0] != out).sum()))
        vs.Stabilizer(device=0, lag=6).set_deblur(3, p)
    st = vs.Stabilizer(device=0, lag=6)
    for sens, mr in ((below(2.0 ** -96), 4.0), (1.0, above(2.0 ** 50)), (below(2.0 ** 6), 1.0e18), (1e-30, 1e18), (1e-38, 4.0), (2.0, above(1.0e18)), (above(3.0e38), 4.0)):
        assert not HM.params_accepted(sens, mr), (sens, mr)
        p = vs.deblur_params(sensitivity=sens, max_ratio=mr)
        with pytest.raises(vs.VsError, match="error -1"):
            vs.bgr_deblur_batch(src, S, cf, ct, params=p, fmt=vs.FMT_BGR16_FULL)
        with pytest.raises(vs.VsError, match="error -1"):
            st.set_deblur(3, p)
        with pytest.raises(vs.VsError, match="error -1"):
            vs.Stabilizer(device=0, lag=6, deblur=3, deblur_params=p)
    assert st.deblur() == 0


K_SLOTS = 1 << 15                                                    # the parameter ring's slots (the group sizes)


@pytest.mark.parametrize("n_cand,extra", [(16, 3), (2, 1)])
def test_the_second_group_of_a_long_call(gpu_vs, n_cand, extra):
    """vs_bgr_deblur_batch uploads candidate entries and ratios in groups of (kSlots / 2 / 5) / n_cand output frames: 204 at 16 candidates,
    1638 at 2.  n_out = group + extra crosses the seam: the second group's destination offset, ring spans and its own aligned / unaligned
    decision.  Frames of 12 x 9 with an odd gap between them: the first group's targets all start on dwords (the x4 kernel), the second
    group has one that does not (the per-sample kernel)"""
    vs = gpu_vs
    group = (K_SLOTS // 2 // 5) // n_cand
    assert group == {16: 204, 2: 1638}[n_cand]
    n_out = group + extra
    assert n_out > group
    w, h, n_src = 12, 9, 8
    rng = np.random.default_rng(n_cand)
    src = HM.contrast_stack(rng, n_src, w, h, np.uint8, 255)
    S = R.sharpness_batch(src, 8)
    assert all(S[i] < S[i + 1] for i in range(n_src - 1))
    cf = np.empty((n_out, n_cand), np.int32)
    cf[:, 0] = 2 * rng.integers(0, 3, n_out)                          # targets 0, 2, 4 ...
    cf[:, 1:] = rng.integers(0, n_src, (n_out, n_cand - 1))
    cf[group - 2:, -1] = 7                                           # ... with the sharpest frame among the candidates on both sides of the seam
    cf[group + extra - 1, 0] = 3                                     # ... and one odd target in the second group
    gap = 4 * ((h * 3 * w + 3) // 4) - h * 3 * w + 2                 # frame stride = 2 mod 4 bytes: even frames on dwords, odd ones not
    assert (h * 3 * w + gap) % 4 == 2
    for o in range(group - 2, n_out):
        assert (S[cf[o, 1:]] > S[cf[o, 0]]).any(), o
    maps = [[(0.0, 0.0, 0.0, 0.0)] + [HM._rot(rng, w, h, big=c % 2 == 0) for c in range(n_cand - 1)] for _ in range(n_out)]
    ct = HM.transforms(vs, maps)
    want = _ref_batch(vs, src, S, cf, ct, 8, 255)
    assert all(not np.array_equal(want[o], src[cf[o, 0]]) for o in range(group - 2, n_out))
    got = _dev_call(vs, src, S, cf, ct, vs.FMT_BGR8, src_gap=gap)
    bad = [o for o in range(n_out) if not np.array_equal(got[o], want[o])]
    assert not bad, (bad[:8], len(bad))
    assert np.array_equal(vs.bgr_deblur_batch(src, S, cf, ct), want)                               # the host-memory form


@pytest.mark.parametrize("w", [4, 5], ids=["4x3_x4", "5x3"])
def test_sharpness_of_more_frames_than_a_grid_has_rows(gpu_vs, w):
    """65 538 frames: the launcher walks gridDim.y in steps of 65 535, so the last three frames belong to a second launch"""
    vs = gpu_vs
    n, h = 65538, 3
    rng = np.random.default_rng(w)
    src = rng.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    want = R.sharpness_many(src, 8)
    assert np.array_equal(want[:50], R.sharpness_batch(src[:50], 8))
    tail = [int(v) for v in want[-3:]]
    assert len(set(tail)) == 3 and min(tail) > 0
    got = vs.sharpness_batch(src)
    assert np.array_equal(got, want), (int((got != want).sum()), got[-3:], want[-3:])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_kernel_against_the_direct_form(gpu_vs, fmt):
    """the kernels' output against the rule written directly in float64 (tests/_deblur_direct.py): at most 1 LSB from round(direct), and a
    difference only where the float64 quotient lies within the fp32 error bound of a .5 boundary; the share of differing samples inside
    the gate tests/test_hostile_cpu.py measured for the restatement"""
    import test_hostile_cpu as TC
    vs = gpu_vs
    code, dtype, bits = FORMATS[fmt]
    maxv = (1 << bits) - 1
    differ = total = 0
    for w, h in HM.DEBLUR_SHAPES:                                    # (the shapes of the CPU measurement: the same samples)
        src, S, cf, maps = HM.deblur_case(vs, fmt, w, h, direct=True)
        ct = HM.transforms(vs, maps)
        got = _dev_call(vs, src, S, cf, ct, code)
        for o in range(len(cf)):
            nd, bad = D.compare(D.deblur_frame(src, S, list(cf[o]), ct[o], bits), got[o], maxv)
            assert bad == 0, (w, h, o, nd, bad)
            differ += nd
            total += got[o].size
    print("%s: %d of %d samples differ between round(direct) and the kernels (share %.3g)" % (fmt, differ, total, differ / total))
    assert differ <= TC.DIRECT_SHARE_GATE[fmt] * total
