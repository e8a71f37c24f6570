"""The quadrant-glyph frames on the GPU: k_tonemap_quadrants and k_fit_quadrants alone through their hooks on inputs no frame produces, the
quadrant streams' kernels on given glyph and colour planes, the frames of ycge_render_frame_quadrants / _ansi_quad / _ansi_quad_delta on
the Cornell box beside a twin context, layers, and the state rules - all against tests/quadrant_restatement.py.  Sub-cell colours are
compared bit for bit (every NaN counted equal to every NaN), glyphs, bytes, out_info and the returned composites exactly, every stream
with its exact length and a canary behind it."""
import ctypes as C

import numpy as np
import pytest

import ansi_layers_restatement as LR
import ansi_rgb_restatement as R
import parity_util as pu
import post_probe_inputs as ppi
import quadrant_restatement as Q
import test_gpu_ansi_stream as S
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import ConsoleLayer, RaytraceRenderer

pytestmark = pytest.mark.gpu
f32 = np.float32
U8P, U16P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
CANARY = S.CANARY
DIGIT_EDGES = np.array([0, 9, 10, 99, 100, 255], np.uint8)
UNITS = np.array(sorted(set(Q.GLYPHS)), np.uint16)


def _hook(g, name):
    fn = getattr(g.L, name)
    fn.restype, fn.argtypes = abi.QUADRANT_HOOK_PROTOTYPES[name]
    return fn


def hook_sdr(g, hdr, fbW, fbH, ss, exposure):
    hdr = np.ascontiguousarray(hdr, f32)
    assert hdr.shape == (fbH * 2 * ss, fbW * ss, 3)
    out = np.full((fbH, fbW, 4, 3), 7.0, f32)
    g._check(_hook(g, "ycge_test_quadrant_sdr")(g.ctx, hdr.ctypes.data, fbW, fbH, ss, float(exposure), out.ctypes.data))
    return out


def hook_fit(g, quad, min_contrast=0):
    """-> (glyphs (n,), fg (n, 3), bg (n, 3)); alpha is 255 everywhere"""
    quad = np.ascontiguousarray(quad, f32).reshape(-1, 12)
    n = quad.shape[0]
    glyphs, rgba = np.zeros(n, np.uint16), np.zeros((2, n, 4), np.uint8)
    g._check(_hook(g, "ycge_test_quadrant_fit")(g.ctx, quad.ctypes.data, n, int(min_contrast), glyphs.ctypes.data, rgba.ctypes.data))
    assert (rgba[..., 3] == 255).all()
    return glyphs, rgba[0, :, :3], rgba[1, :, :3]


def check_fit(g, quad, min_contrast=0, what=""):
    glyphs, fg, bg = hook_fit(g, quad, min_contrast)
    wg, wfg, wbg, masks = Q.fit(quad, min_contrast)
    bad = np.flatnonzero((glyphs != wg) | (fg != wfg).any(axis=1) | (bg != wbg).any(axis=1))
    assert bad.size == 0, (what, min_contrast, bad[:4], np.asarray(quad).reshape(-1, 12)[bad[:2]], glyphs[bad[:2]], wg[bad[:2]], fg[bad[:2]], wfg[bad[:2]])
    return masks


def hook_stream(g, glyphs, rgba, cw, ch, vp=(0, 0), fg=7, bg=0, clear=False):
    glyphs, rgba = np.ascontiguousarray(glyphs, np.uint16), np.ascontiguousarray(rgba, np.uint8)
    fbH, fbW = glyphs.shape
    cap = RaytraceRenderer.ansi_rgb_stream_bound(cw, ch, g.L)
    out, n = np.full(cap + 64, CANARY, np.uint8), C.c_size_t(0)
    g._check(_hook(g, "ycge_test_ansi_quad_stream")(g.ctx, glyphs.ctypes.data_as(U16P), rgba.ctypes.data_as(U8P), fbW, fbH, cw, ch, vp[0], vp[1], fg, bg, int(clear),
                                                    out.ctypes.data_as(U8P), cap, C.byref(n)))
    assert n.value <= cap and (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes()


def hook_delta(g, shown, glyphs, rgba, cw, ch, vp=(0, 0), fg=7, bg=0, clear=False, gap=3, tol=0):
    """shown: (glyphs, colours) of the console, or None -> (stream, info, next shown)"""
    glyphs, rgba = np.ascontiguousarray(glyphs, np.uint16), np.ascontiguousarray(rgba, np.uint8)
    fbH, fbW = glyphs.shape
    cap = RaytraceRenderer.ansi_rgb_stream_bound(cw, ch, g.L)
    out, n, info = np.full(cap + 64, CANARY, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    sg = sc = None
    if shown is not None:
        sg, sc = np.ascontiguousarray(shown[0], np.uint16), np.ascontiguousarray(shown[1], np.uint8)
    ng, nc = np.full((ch, cw), 0x5A5A, np.uint16), np.full((2 * ch, cw, 4), 0x5A, np.uint8)
    g._check(_hook(g, "ycge_test_ansi_quad_delta")(g.ctx, sc.ctypes.data_as(U8P) if shown is not None else None, sg.ctypes.data_as(U16P) if shown is not None else None,
                                                   glyphs.ctypes.data_as(U16P), rgba.ctypes.data_as(U8P), fbW, fbH, cw, ch, vp[0], vp[1], fg, bg, int(clear), gap, tol,
                                                   out.ctypes.data_as(U8P), cap, C.byref(n), info, nc.ctypes.data_as(U8P), ng.ctypes.data_as(U16P)))
    assert n.value <= cap and (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), dict(zip(R.INFO, (int(v) for v in info))), (ng, nc)


def check_delta(g, shown, glyphs, rgba, cw, ch, vp=(0, 0), fg=7, bg=0, gap=3, tol=0, what=""):
    got, info, nxt = hook_delta(g, shown, glyphs, rgba, cw, ch, vp, fg, bg, False, gap, tol)
    want, winfo, wnxt = Q.delta(shown, glyphs, rgba, cw, ch, vp, fg, bg, gap, tol)
    S.assert_stream(got, want, what)
    assert info == winfo, (what, info, winfo)
    assert (nxt[0] == wnxt[0]).all() and (nxt[1] == wnxt[1]).all(), (what, "next shown")
    return got, info, nxt


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------------------------- 1: k_tonemap_quadrants alone
@pytest.mark.parametrize("fbw,fbh,ss", [(1, 1, 2), (7, 3, 2), (257, 3, 2), (5, 2, 4), (3, 2, 6)])
def test_sub_cell_colours_bit_for_bit(enc, fbw, fbh, ss):
    """drawn HDR, then the post probe's special values - NaN, +-inf, negatives, denormals, 1e30, FLT_MAX - each in one sample of one quadrant,
    in one channel or in all three; (257, 3, 2): a row of chexels across a workgroup's edge (64 chexels a workgroup)"""
    rng = np.random.default_rng([fbw, fbh, ss])
    H, W = fbh * 2 * ss, fbw * ss
    hdr = rng.uniform(0, 2.5, (H, W, 3)).astype(f32)
    hdr[rng.random((H, W)) < 0.1] = 0
    for exposure in (1.0, 0.37):
        got = hook_sdr(enc, hdr, fbw, fbh, ss, exposure)
        assert ppi.nan_aware_mismatches(got, Q.sub_cells(hdr, fbw, fbh, ss, exposure)) == 0, (fbw, fbh, ss, exposure)
    specials = ppi.NONFINITE_SPECIALS + ppi.FINITE_SPECIALS
    cells = [(cy, cx) for cy in range(fbh) for cx in range(fbw)]
    for j, v in enumerate(specials * 2):
        cy, cx = cells[(j * 7) % len(cells)]
        k = j % 4
        y = (cy * 2 + k // 2) * ss + int(rng.integers(0, ss))
        x = cx * ss + (k % 2) * (ss // 2) + int(rng.integers(0, ss // 2))
        if j < len(specials):
            hdr[y, x, j % 3] = v
        else:
            hdr[y, x, :] = v
    got = hook_sdr(enc, hdr, fbw, fbh, ss, 0.8)
    want = Q.sub_cells(hdr, fbw, fbh, ss, 0.8)
    assert ppi.nan_aware_mismatches(got, want) == 0, (fbw, fbh, ss, "specials")
    assert fbw * fbh < 4 or np.isnan(want).any() or (want == 1).any()


def test_sub_cell_hook_refusals(enc):
    out, hdr = np.zeros(12, f32), np.zeros(2 * 6 * 3 * 3, f32)
    fn = _hook(enc, "ycge_test_quadrant_sdr")
    for ss in (1, 3, 0, -2, 66):
        assert fn(enc.ctx, hdr.ctypes.data, 1, 1, ss, 1.0, out.ctypes.data) == abi.YCGE_ERR_INVALID_ARG and b"super_sample %d" % ss in enc.L.ycge_last_error(enc.ctx)
    assert fn(enc.ctx, None, 1, 1, 2, 1.0, out.ctypes.data) == abi.YCGE_ERR_INVALID_ARG and not out.any()


# ------------------------------------------------------------------------------------------------------------- 2: k_fit_quadrants alone
@pytest.fixture(scope="module")
def byte_values(product_lib):
    """float_of[k]: a binary32 whose LinearToSrgb8 byte is k - the library's own thresholds (the smallest such value), 0 for byte 0"""
    t32, t64 = np.zeros(255, f32), np.zeros(255, np.float64)
    fn = product_lib.ycge_host_srgb_thresholds
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    assert fn(t32.ctypes.data, t64.ctypes.data) == 0
    float_of = np.concatenate([[f32(0)], t32]).astype(f32)
    assert np.array_equal(R.CR.srgb8_v(float_of.astype(np.float64)), np.arange(256))
    return float_of


@pytest.fixture(scope="module")
def drawn_cells():
    rng = np.random.default_rng(100000)
    cells = rng.random((100000, 12)).astype(f32)
    near = np.clip(rng.random((30000, 1, 3)) + rng.uniform(-0.02, 0.02, (30000, 4, 3)), 0, 1).astype(f32).reshape(-1, 12)          # nearly flat: the contrast rule decides
    cells[::3][:30000] = near
    return cells


def test_fit_greys_and_built_ties(enc, byte_values):
    vals = (0, 1, 2, 127, 128, 254, 255)
    greys = np.array([[[byte_values[v]] * 3 for v in q] for q in np.stack(np.meshgrid(*[vals] * 4, indexing="ij"), -1).reshape(-1, 4)], f32)
    assert greys.shape == (2401, 4, 3)
    for mc in (0, 1, 8, 255):
        masks = check_fit(enc, greys, mc, "greys")
        assert mc != 255 or not masks.any()
    assert set(check_fit(enc, greys, 0).tolist()) == set(range(8))
    rng = np.random.default_rng(3)
    ties = []
    for _ in range(200):
        a, b, c = (byte_values[rng.integers(0, 256, 3)] for _ in range(3))
        ties += [[a, a, b, b], [a, b, a, b], [a, b, b, a], [b, a, a, b],                     # complementary pairs
                 [a, a, a, b], [a, a, b, a], [a, b, a, a], [b, a, a, a],                     # three equal
                 [a, a, b, c], [a, b, a, c], [b, c, a, a], [a, b, c, a], [a, a, a, a]]       # two equal, all equal
    ties = np.array(ties, f32)
    masks = check_fit(enc, ties, 0, "ties")
    assert set(masks.tolist()) == set(range(8))
    check_fit(enc, ties, 8, "ties, min_contrast 8")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_fit_sizes(enc, drawn_cells, n):
    check_fit(enc, drawn_cells[-n:], 0, n)
    check_fit(enc, drawn_cells[:n], 8, n)


@pytest.mark.parametrize("mc", [0, 1, 8, 255])
def test_fit_100000_drawn_cells(enc, drawn_cells, mc):
    masks = check_fit(enc, drawn_cells, mc, "drawn")
    if mc < 255:
        # (every two-colour mask occurs; the one-colour mask needs a flat cell, which the contrast rule makes of the nearly flat ones)
        assert set(range(1, 8)) <= set(masks.tolist()) and (mc == 0 or (masks == 0).sum() > 0)
    else:
        assert not masks.any()


def test_fit_inputs_outside_the_unit_interval(enc):
    rng = np.random.default_rng(9)
    odd = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 2.0, 1e30, -1e30, 1e-40, 1.0, 0.0, 0.5, 0.0031308, 0.00313081], f32)
    cells = rng.choice(odd, (4000, 12))
    cells[::2, 6:] = rng.random((2000, 6)).astype(f32)
    for mc in (0, 8):
        check_fit(enc, cells, mc, "odd inputs")
    g, fg, bg = hook_fit(enc, np.full((1, 12), np.nan, f32))
    assert g[0] == 0x2580 and not fg.any() and not bg.any()


def test_fit_hook_refusals(enc):
    q, g = np.zeros(12, f32), np.zeros(1, np.uint16)
    fn = _hook(enc, "ycge_test_quadrant_fit")
    for n, mc, word in ((0, 0, b"n = 0"), (1, -1, b"min_contrast = -1"), (1, 256, b"min_contrast = 256")):
        assert fn(enc.ctx, q.ctypes.data, n, mc, g.ctypes.data, None) == abi.YCGE_ERR_INVALID_ARG and word in enc.L.ycge_last_error(enc.ctx)
    assert fn(enc.ctx, q.ctypes.data, 1, 0, None, None) == abi.YCGE_ERR_INVALID_ARG and not g.any()


# ------------------------------------------------------------------------------------------------------------- 3: the stream kernels alone
def _planes(rng, h, w):
    """glyphs with all eight masks' code units, colours in runs of three equal columns whose channels sit on the digit boundaries"""
    glyphs = rng.choice(UNITS, (h, w)).astype(np.uint16)
    glyphs.flat[:min(glyphs.size, len(Q.GLYPHS))] = Q.GLYPHS[:min(glyphs.size, len(Q.GLYPHS))]
    cols = DIGIT_EDGES[rng.integers(0, 6, (2 * h, (w + 2) // 3, 3))]
    rgba = np.empty((2 * h, w, 4), np.uint8)
    rgba[..., :3] = np.repeat(cols, 3, axis=1)[:, :w]
    rgba[..., 3] = rng.integers(0, 256, (2 * h, w))
    return glyphs, rgba


def _next_frame(rng, glyphs, rgba, density):
    """`density` of the cells redrawn (glyph and colours), a third of the others moved by -2..2 in one channel"""
    g, p = glyphs.copy(), rgba.copy()
    if density > 0:
        h, w = g.shape
        jitter = rng.integers(-2, 3, (2 * h, w, 3)) * (rng.random((2 * h, w, 1)) < 1 / 3)
        p[..., :3] = np.clip(p[..., :3].astype(np.int64) + jitter, 0, 255)
        redraw = rng.random((h, w)) < density
        g[redraw] = rng.choice(UNITS, int(redraw.sum()))
        both = np.repeat(redraw, 2, axis=0)
        p[both, :3] = rng.integers(0, 256, (int(both.sum()), 3))
    return g, p


@pytest.mark.parametrize("cw,ch", [(7, 3), (1100, 3), (33, 70)])
def test_hook_full_stream_and_deltas(enc, cw, ch):
    rng = np.random.default_rng(cw * 100 + ch)
    glyphs, rgba = _planes(rng, ch, cw)
    for clear in (False, True):
        got = hook_stream(enc, glyphs, rgba, cw, ch, clear=clear)
        S.assert_stream(got, Q.stream(glyphs, rgba, cw, ch, clear=clear), (cw, ch, clear))
    assert all(LR.utf8(int(u)) in got for u in UNITS)
    key, info, shown = check_delta(enc, None, glyphs, rgba, cw, ch, what="keyframe")
    S.assert_stream(key, Q.stream(glyphs, rgba, cw, ch), "the keyframe is the full stream")
    assert info["keyframe"] == 1
    few = 3.0 / (cw * ch)
    for k, (density, tol, gap) in enumerate([(0.0, 0, 3), (few, 0, 0), (few, 2, 8), (1.0, 0, 3), (1.0, 2, 0), (0.3, 2, 3), (0.3, 0, 8)]):
        g2, p2 = _next_frame(rng, glyphs, rgba, density)
        got, info, _ = check_delta(enc, shown, g2, p2, cw, ch, gap=gap, tol=tol, what=(cw, ch, density, tol, gap))
        assert density > 0 or info == dict(keyframe=0, changed=0, emitted=1, runs=1)
        assert density < 1 or info["emitted"] == cw * ch


@pytest.mark.parametrize("vp", [(0, 0), (-4, 0), (0, -2), (6, 0), (0, 3), (-3, -1), (5, 2), (-100, 0), (0, 40)])
def test_hook_viewport_off_each_edge(enc, vp):
    rng = np.random.default_rng(abs(vp[0] * 31 + vp[1]) + 1)
    cw, ch = 17, 6
    glyphs, rgba = _planes(rng, 5, 14)
    S.assert_stream(hook_stream(enc, glyphs, rgba, cw, ch, vp, 3, 12, True), Q.stream(glyphs, rgba, cw, ch, vp, 3, 12, True), vp)
    _, _, shown = check_delta(enc, None, glyphs, rgba, cw, ch, vp, 3, 12, what=(vp, "keyframe"))
    g2, p2 = _next_frame(rng, glyphs, rgba, 0.2)
    check_delta(enc, shown, g2, p2, cw, ch, vp, 3, 12, gap=2, tol=1, what=(vp, "delta"))


def test_hook_chain_of_three_frames_against_what_is_shown(enc):
    rng = np.random.default_rng(77)
    cw, ch, vp, tol = 40, 9, (2, 1), 2
    glyphs, rgba = _planes(rng, 7, 36)
    screen, shown = LR.Screen(cw, ch), None
    for k in range(4):
        got, info, shown = check_delta(enc, shown, glyphs, rgba, cw, ch, vp, gap=k % 4, tol=tol, what=("chain", k))
        assert info["keyframe"] == int(k == 0)
        screen.feed(got)
        full = LR.Screen(cw, ch).feed(Q.stream(glyphs, rgba, cw, ch, vp))
        assert R.within(screen, full, tol), k
        glyphs, rgba = _next_frame(rng, glyphs, rgba, 0.15)


def test_hook_a_glyph_change_alone_is_emitted(enc):
    rng = np.random.default_rng(5)
    cw, ch = 12, 4
    glyphs, rgba = _planes(rng, ch, cw)
    _, _, shown = check_delta(enc, None, glyphs, rgba, cw, ch)
    g2, p2 = glyphs.copy(), rgba.copy()
    g2[2, 5] = 0x259E if glyphs[2, 5] != 0x259E else 0x2598
    p2[4, 5, 0] = np.clip(int(p2[4, 5, 0]) + (1 if p2[4, 5, 0] < 255 else -1), 0, 255)          # within the tolerance
    got, info, nxt = check_delta(enc, shown, g2, p2, cw, ch, gap=0, tol=2, what="glyph only")
    assert info == dict(keyframe=0, changed=1, emitted=2, runs=2) and LR.utf8(int(g2[2, 5])) in got
    assert nxt[0][2, 5] == g2[2, 5] and nxt[1][4, 5, 0] == p2[4, 5, 0]          # shown = cur for the emitted cell


def test_stream_hook_refusals(enc):
    glyphs, rgba = _planes(np.random.default_rng(1), 2, 3)
    cap = RaytraceRenderer.ansi_rgb_stream_bound(3, 2, enc.L)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    fn = _hook(enc, "ycge_test_ansi_quad_stream")
    call = lambda gl, c=cap, fg=7: fn(enc.ctx, gl, rgba.ctypes.data_as(U8P), 3, 2, 3, 2, 0, 0, fg, 0, 0, out.ctypes.data_as(U8P), c, C.byref(n))
    for args, word in (((None,), b"bad framebuffer"), ((glyphs.ctypes.data_as(U16P), cap - 1), b"capacity %d" % (cap - 1)), ((glyphs.ctypes.data_as(U16P), cap, 16), b"16")):
        assert call(*args) == abi.YCGE_ERR_INVALID_ARG and word in enc.L.ycge_last_error(enc.ctx)
    assert not out.any() and n.value == 0
    assert call(glyphs.ctypes.data_as(U16P)) == 0 and n.value > 0


# ------------------------------------------------------------------------------------------------------------- 4: frames
FBW, FBH, CW, CH, VP = 80, 45, 84, 47, (2, 1)


def frame_planes(g, min_contrast=0):
    """the restatement's planes of the frame g rendered last: sub_cells of its denoised buffer under its exposure, then the fit"""
    quad = Q.sub_cells(g.read(abi.BUF_DENOISED), g.fbW, g.fbH, g.ss, g.stats.exposure)
    return (quad,) + Q.planes(quad, g.fbW, g.fbH, min_contrast)


@pytest.fixture(params=[2, 4], ids=["ss2", "ss4"])
def pair(request, product_lib):
    a, b, pose = S.twins(1, FBW, FBH, request.param)
    yield a, b, pose
    a.close(); b.close()


def same_frame_state(a, b, what):
    assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure, what
    assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY)), what


def test_frames_planes(pair):
    a, b, pose = pair
    seen = set()
    for k in range(3):
        S.move((a, b), pose, k)
        plain = a.TryFlipAndBlit(want_sdr=True)
        mc = (0, 0, 4)[k]
        out = b.TryFlipAndBlitQuadrants(quad_sdr=True, glyphs=True, rgba=True, sdr=True, min_contrast=mc)
        assert pu.bits_equal(plain, out["sdr"]), k
        same_frame_state(a, b, k)
        quad, glyphs, rgba = frame_planes(b, mc)
        assert ppi.nan_aware_mismatches(out["quad_sdr"], quad) == 0, k
        assert np.array_equal(out["glyphs"], glyphs) and np.array_equal(out["rgba"], rgba), k
        seen |= set(out["glyphs"].ravel().tolist())
    assert len(seen) >= 5 and 0x20 not in seen          # (a picture, not one flat colour)
    # any subset of the destinations: the glyphs alone, the SDR alone
    S.move((a, b), pose, 3)
    plain = a.TryFlipAndBlit(want_sdr=True)
    only = b.TryFlipAndBlitQuadrants(glyphs=True, rgba=False)
    assert list(only) == ["glyphs"] and np.array_equal(only["glyphs"], frame_planes(b)[1])
    S.move((a, b), pose, 4)
    plain = a.TryFlipAndBlit(want_sdr=True)
    only = b.TryFlipAndBlitQuadrants(glyphs=False, rgba=False, sdr=True)
    assert pu.bits_equal(plain, only["sdr"])
    same_frame_state(a, b, "subsets")


def test_frames_streams(pair):
    a, b, pose = pair
    c = RaytraceRenderer(b.flat, FBW, FBH, pose.get("fov", 45.0), b.ss)
    c.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    try:
        tol, shown, screen = 2, None, LR.Screen(CW, CH)
        for k in range(3):
            S.move((a, b, c), pose, k)
            plain = a.TryFlipAndBlit(want_sdr=True)
            full, sdr = b.TryFlipAndBlitAnsiQuad(CW, CH, VP, 3, 12, clear_screen=(k == 0), sdr=True)
            assert pu.bits_equal(plain, sdr), k
            _, glyphs, rgba = frame_planes(b)
            S.assert_stream(full, Q.stream(glyphs, rgba, CW, CH, VP, 3, 12, clear=(k == 0)), ("full", k))
            stream, info, sdr = c.TryFlipAndBlitAnsiQuadDelta(CW, CH, VP, 3, 12, merge_gap=2, tolerance=tol, sdr=True)
            assert pu.bits_equal(plain, sdr), k
            want, winfo, shown = Q.delta(shown, glyphs, rgba, CW, CH, VP, 3, 12, gap=2, tol=tol)
            S.assert_stream(stream, want, ("delta", k))
            assert info == winfo and info["keyframe"] == int(k == 0), (k, info, winfo)
            if k == 0:
                S.assert_stream(stream, Q.stream(glyphs, rgba, CW, CH, VP, 3, 12), "the first delta is the keyframe: the full stream")
            screen.feed(stream)
            assert R.within(screen, LR.Screen(CW, CH).feed(Q.stream(glyphs, rgba, CW, CH, VP, 3, 12)), tol), k
            same_frame_state(a, b, k); same_frame_state(a, c, k)
    finally:
        c.close()


def console_layers(k):
    """a console-sized text framebuffer below the raytrace one, blank but for one row, and a 10 x 4 one above"""
    chars = np.full((CH, CW), 0x20, np.uint16)
    chars[CH - 1] = [ord(ch) for ch in f"frame {k} ▌▛ éΩ".replace(" ", "_").ljust(CW, "_")[:CW]]
    menu = np.full((4, 10), ord("+"), np.uint16)
    menu[1:3, 1:9] = [ord(ch) for ch in "menu_" + str(k % 10) + "__"]
    menu[2, 3:5] = 0x20
    return [LR.Layer(chars, (1.0, 1.0, 1.0), (0.0, 0.0, 0.5)), LR.Layer(menu, (1.0, 1.0, 0.0), (0.5, 0.5, 0.5), 30 + k, 2)]


def mirror(layers):
    return [ConsoleLayer(l.chars, l.fg, l.bg, l.x, l.y) for l in layers]


def test_layers_take_the_fitted_cells(product_lib):
    a, b, pose = S.twins(1, FBW, FBH, 2)
    try:
        shown = None
        for k in range(3):
            S.move((a, b), pose, k)
            layers = console_layers(k)
            a.SetConsoleLayers(mirror(layers), 1); b.SetConsoleLayers(mirror(layers), 1)
            full = a.TryFlipAndBlitAnsiQuad(CW, CH, VP, 3, 12)
            _, glyphs, rgba = frame_planes(a)
            S.assert_stream(full, Q.stream(glyphs, rgba, CW, CH, VP, 3, 12, layers=layers, raytrace_at=1), ("layered full", k))
            assert ("frame_%d" % k).encode() in full and ("menu_%d" % k).encode() in full
            stream, info = b.TryFlipAndBlitAnsiQuadDelta(CW, CH, VP, 3, 12, merge_gap=1, tolerance=1)
            want, winfo, shown = Q.delta(shown, glyphs, rgba, CW, CH, VP, 3, 12, gap=1, tol=1, layers=layers, raytrace_at=1)
            S.assert_stream(stream, want, ("layered delta", k))
            assert info == winfo and info["keyframe"] == int(k == 0), (k, info, winfo)
        b.SetConsoleLayers([], 0)          # n -> 0: a keyframe, the bytes of the unlayered stream
        stream, info = b.TryFlipAndBlitAnsiQuadDelta(CW, CH, VP, 3, 12, merge_gap=1, tolerance=1)
        _, glyphs, rgba = frame_planes(b)
        assert info["keyframe"] == 1
        S.assert_stream(stream, Q.stream(glyphs, rgba, CW, CH, VP, 3, 12), "n == 0")
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 5: state and refusals
def quad_step(g, shown, keyframe_expected, what, tol=0, **kw):
    """one _quad_delta frame of g held to the restatement against `shown`; -> the next shown"""
    stream, info = g.TryFlipAndBlitAnsiQuadDelta(CW, CH, VP, 3, 12, merge_gap=2, tolerance=tol, **kw)
    _, glyphs, rgba = frame_planes(g, kw.get("min_contrast", 0))
    want, winfo, nxt = Q.delta(None if keyframe_expected else shown, glyphs, rgba, CW, CH, VP, 3, 12, gap=2, tol=tol)
    S.assert_stream(stream, want, what)
    assert info == winfo and info["keyframe"] == int(keyframe_expected), (what, info, winfo)
    return nxt


@pytest.fixture()
def one(product_lib):
    a, b, pose = S.twins(1, FBW, FBH, 2)
    a.close()
    yield b
    b.close()


def test_the_three_families_invalidate_each_other_and_resize_keyframes(one):
    g = one
    s = quad_step(g, None, True, "first")
    s = quad_step(g, s, False, "delta")
    s = quad_step(g, s, False, "min_contrast is no part of the key", min_contrast=6)
    _, info = g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)
    assert info["keyframe"] == 1, "a 24-bit delta after a quad delta"
    s = quad_step(g, s, True, "a quad delta after a 24-bit delta")
    _, info = g.TryFlipAndBlitAnsiDelta(CW, CH, VP, 3, 12)
    assert info["keyframe"] == 1, "a 256-colour delta after a quad delta"
    s = quad_step(g, s, True, "a quad delta after a 256-colour delta")
    s = quad_step(g, s, False, "delta")
    g.TryFlipAndBlitAnsiQuad(CW, CH, VP, 3, 12)
    s = quad_step(g, s, True, "after a full quad stream")
    _, info = g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)
    assert info["keyframe"] == 1
    _, info = g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)
    assert info["keyframe"] == 0
    g.TryFlipAndBlitAnsiQuad(CW, CH, VP, 3, 12)
    _, info = g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)
    assert info["keyframe"] == 1, "a 24-bit delta after a full quad stream"
    s = quad_step(g, None, True, "again")
    g.Resize(FBW, FBH, 2)
    s = quad_step(g, s, True, "after ycge_resize")
    s = quad_step(g, s, False, "delta")
    quad_step(g, s, True, "keyframe asked", keyframe=True)


def test_refusals_leave_the_context_and_the_delta_state(one):
    g = one
    L = g.L
    s = quad_step(g, None, True, "first")
    frame0 = g.stats.frame
    cap = RaytraceRenderer.ansi_rgb_stream_bound(CW, CH, L)
    out, n, info = np.zeros(cap, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    p = out.ctypes.data_as(U8P)
    glyphs = np.zeros((FBH, FBW), np.uint16)
    full = lambda mc=0, c=cap, fg=3, o=p, ln=C.byref(n): L.ycge_render_frame_ansi_quad(g.ctx, CW, CH, VP[0], VP[1], fg, 12, 0, mc, o, c, ln, None, None)
    delta = lambda mc=0, c=cap, gap=2, tol=0: L.ycge_render_frame_ansi_quad_delta(g.ctx, CW, CH, VP[0], VP[1], 3, 12, 0, gap, tol, 0, mc, p, c, C.byref(n), info, None, None)
    planes = lambda mc=0, gl=glyphs.ctypes.data_as(U16P): L.ycge_render_frame_quadrants(g.ctx, None, None, gl, None, mc, None)
    for call, words in [(lambda: full(-1), [b"min_contrast -1"]), (lambda: full(256), [b"min_contrast 256"]), (lambda: delta(-1), [b"min_contrast -1"]),
                        (lambda: delta(256), [b"min_contrast 256"]), (lambda: planes(-1), [b"min_contrast -1"]), (lambda: planes(256), [b"min_contrast 256"]),
                        (lambda: planes(0, None), [b"every destination is NULL"]), (lambda: full(0, cap - 1), [b"capacity %d" % (cap - 1)]),
                        (lambda: delta(0, cap - 1), [b"capacity %d" % (cap - 1)]), (lambda: full(0, cap, 16), [b"16"]), (lambda: full(0, cap, 3, None), [b"NULL"]),
                        (lambda: full(0, cap, 3, p, None), [b"NULL"]), (lambda: delta(0, cap, 9), [b"merge_gap 9"]), (lambda: delta(0, cap, 2, 256), [b"tolerance 256"])]:
        rc = call()
        msg = L.ycge_last_error(g.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), msg
    assert not out.any() and n.value == 0 and list(info) == [9, 9, 9, 9] and not glyphs.any() and g.stats.frame == frame0
    s = quad_step(g, s, False, "a refused call forces no keyframe")
    assert g.stats.frame == frame0 + 1


@pytest.mark.parametrize("ss", [1, 3])
def test_an_odd_super_sample_is_refused(product_lib, ss):
    a, g, pose = S.twins(1, 16, 8, ss)
    a.close()
    try:
        _, info = g.TryFlipAndBlitAnsiRgbDelta(16, 8)
        assert info["keyframe"] == 1
        frame0 = g.stats.frame
        for call in (lambda: g.TryFlipAndBlitQuadrants(), lambda: g.TryFlipAndBlitAnsiQuad(16, 8), lambda: g.TryFlipAndBlitAnsiQuadDelta(16, 8)):
            with pytest.raises(abi.YcgeError) as e:
                call()
            assert e.value.status == abi.YCGE_ERR_INVALID_ARG and f"super_sample {ss}" in str(e.value), str(e.value)
        _, info = g.TryFlipAndBlitAnsiRgbDelta(16, 8)
        assert info["keyframe"] == 0 and g.stats.frame == frame0 + 1, "the refusals left the context and its delta state alone"
        g.Resize(16, 8, 2)
        assert set(g.TryFlipAndBlitQuadrants()) == {"glyphs", "rgba"}
    finally:
        g.close()


def test_a_peer_context_is_refused(product_lib):
    a, b, pose = S.twins(2, 160, 45, 2, devices=[0, 0, 0])
    try:
        fn = b.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int32]
        peer = fn(b.ctx, 0)
        assert peer
        cap = RaytraceRenderer.ansi_rgb_stream_bound(160, 45, b.L)
        out, n, glyphs = np.zeros(cap, np.uint8), C.c_size_t(0), np.zeros((45, 160), np.uint16)
        p = out.ctypes.data_as(U8P)
        for rc in (b.L.ycge_render_frame_quadrants(peer, None, None, glyphs.ctypes.data_as(U16P), None, 0, None),
                   b.L.ycge_render_frame_ansi_quad(peer, 160, 45, 0, 0, 7, 0, 0, 0, p, cap, C.byref(n), None, None),
                   b.L.ycge_render_frame_ansi_quad_delta(peer, 160, 45, 0, 0, 7, 0, 0, 3, 0, 0, 0, p, cap, C.byref(n), None, None, None)):
            assert rc == abi.YCGE_ERR_INVALID_ARG and b"driven by their root" in b.L.ycge_last_error(peer)
        assert not out.any() and not glyphs.any()
    finally:
        a.close(); b.close()
