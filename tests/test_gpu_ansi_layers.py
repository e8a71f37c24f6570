"""The layered ANSI streams on the GPU: the compose and stream kernels through their hook (ycge_test_ansi_layers) on framebuffers, layers and
glyphs no frame produces, in both colour forms, and the eight stream calls behind ycge_console_set_layers - all against the restatement
(tests/ansi_layers_restatement.py) and a terminal model fed every stream in order.  Every stream is compared byte for byte, with its exact
length and a canary behind it; every out_info and every returned composite with the restatement's."""
import ctypes as C

import numpy as np
import pytest

import ansi_layers_restatement as LR
import ansi_rgb_restatement as R
import ansi_stream_restatement as A
import parity_util as pu
import test_gpu_ansi_stream as S
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import ConsoleLayer, RaytraceRenderer, VideoRenderer

pytestmark = pytest.mark.gpu
U8P, U16P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
CANARY = S.CANARY
RED, BLUE, WHITE, GREY = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5)
WIDTHS = np.array([0x41, 0x7F, 0x80, 0x7FF, 0x800, 0x2580, 0xD800, 0xFFFF], np.uint16)          # 1, 1, 2, 2, 3, 3, 3, 3 bytes


def mirror(layers):
    """restatement layers as the Python mirror's"""
    return [ConsoleLayer(l.chars, l.fg, l.bg, l.x, l.y) for l in layers]


def layer_array(layers):
    m = mirror(layers)
    arr = (abi.ConsoleLayer * max(1, len(m)))()
    for k, l in enumerate(m):
        arr[k] = l.as_struct()
    return arr, m


def bound(g, rgb, cw, ch):
    return (RaytraceRenderer.ansi_rgb_stream_bound if rgb else RaytraceRenderer.ansi_stream_bound)(cw, ch, g.L)


def hook(g, rgb, plane, layers, at, cw, ch, vp=(0, 0), fg=7, bg=0, clear=False, delta=False, prev=None, gap=1, tol=0):
    """ycge_test_ansi_layers -> (stream, info or None, (glyphs, colours)): nothing past the stream's length was written"""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    fbH, fbW = (plane.shape[0] // 2, plane.shape[1]) if rgb else plane.shape[:2]
    cap = bound(g, rgb, cw, ch)
    out = np.full(cap + 64, CANARY, np.uint8)
    n, info = C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    colours = np.full((2 * ch, cw, 4) if rgb else (ch, cw, 2), 0x5A, np.uint8)
    glyphs = np.full((ch, cw), 0x5A5A, np.uint16)
    pg = pc = None
    if prev is not None:
        pg, pc = np.ascontiguousarray(prev[0], dtype=np.uint16), np.ascontiguousarray(prev[1], dtype=np.uint8)
        assert pg.shape == glyphs.shape and pc.shape == colours.shape
    arr, keep = layer_array(layers)
    fn = g.L.ycge_test_ansi_layers
    fn.restype, fn.argtypes = abi.ANSI_LAYERS_HOOK_PROTOTYPES["ycge_test_ansi_layers"]
    g._check(fn(g.ctx, int(rgb), plane.ctypes.data_as(U8P), fbW, fbH, arr, len(layers), at, pc.ctypes.data_as(U8P) if prev is not None else None,
                pg.ctypes.data_as(U16P) if prev is not None else None, cw, ch, vp[0], vp[1], fg, bg, int(clear), int(delta), gap, tol, out.ctypes.data_as(U8P), cap,
                C.byref(n), info, colours.ctypes.data_as(U8P), glyphs.ctypes.data_as(U16P)))
    assert n.value <= cap and (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), (dict(zip(LR.INFO, (int(v) for v in info))) if delta else None), (glyphs, colours)


def check_full(g, rgb, plane, layers, at, cw, ch, vp=(0, 0), fg=7, bg=0, clear=False, what=""):
    got, _, comp = hook(g, rgb, plane, layers, at, cw, ch, vp, fg, bg, clear)
    S.assert_stream(got, LR.stream(rgb, plane, layers, at, cw, ch, vp, fg, bg, clear), (what, rgb))
    want = LR.composite(rgb, plane, layers, at, cw, ch, vp, fg, bg)
    assert (comp[0] == want[0]).all() and (comp[1] == want[1]).all(), (what, rgb, "composite")
    return got, comp


def check_delta(g, rgb, prev, plane, layers, at, cw, ch, vp=(0, 0), fg=7, bg=0, gap=1, tol=0, clear=False, what=""):
    got, info, comp = hook(g, rgb, plane, layers, at, cw, ch, vp, fg, bg, clear, True, prev, gap, tol)
    want, winfo, wcomp = LR.delta(rgb, prev, plane, layers, at, cw, ch, vp, fg, bg, gap, tol, clear)
    S.assert_stream(got, want, (what, rgb))
    assert info == winfo, (what, rgb, info, winfo)
    assert (comp[0] == wcomp[0]).all() and (comp[1] == wcomp[1]).all(), (what, rgb, "next composite")
    return got, info, comp


def random_plane(rng, rgb, fbH, fbW):
    return rng.integers(0, 256, (2 * fbH, fbW, 4) if rgb else (fbH, fbW, 2)).astype(np.uint8)


def random_layer(rng, w, h, x, y, units=WIDTHS, holes=1 / 3):
    chars = rng.choice(units, (h, w))
    chars[rng.random((h, w)) < holes] = 0x20
    return LR.Layer(chars, rng.random((h, w, 3)).astype(np.float32), rng.random((h, w, 3)).astype(np.float32), x, y)


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


FORMS = pytest.mark.parametrize("rgb", [False, True], ids=["256", "rgb"])


# ------------------------------------------------------------------------------------------------------------- 1: the kernels alone
@FORMS
@pytest.mark.parametrize("cw,ch", [(1, 1), (2, 1), (5, 2)])
def test_hook_characters_transparency_and_order(enc, rgb, cw, ch):
    rng = np.random.default_rng(cw * 10 + ch)
    rt = random_plane(rng, rgb, 1, 1)
    one = lambda unit, fg=RED, bg=BLUE, x=0, y=0: LR.Layer([[unit]], fg, bg, x, y)
    for unit in (0x00, 0x7F, 0x80, 0x7FF, 0x800, 0xD800, 0xDFFF, 0xFFFF):
        for at, vp in ((0, (0, 0)), (1, (0, 0)), (1, (7, 7))):
            check_full(enc, rgb, rt, [one(unit)], at, cw, ch, vp, what=(hex(unit), at, vp))
    hole = one(0x20, WHITE, RED)
    a, b = one(ord("a"), RED, BLUE), one(ord("b"), BLUE, RED)
    wide = LR.Layer([[ord("x"), ord("y")]], RED, BLUE)
    cases = [([hole], 0, (0, 0)), ([hole], 0, (3, 0)), ([a, b], 0, (0, 0)), ([b, a], 0, (0, 0)), ([a, hole], 0, (0, 0)), ([a, hole], 1, (0, 0)),
             ([a, b], 2, (0, 0)), ([hole, hole], 1, (1, 0)), ([wide], 1, (0, 0)), ([wide], 1, (1, 0)), ([wide], 0, (0, 0)), ([one(0, WHITE, RED)], 0, (0, 0))]
    for layers, at, vp in cases:
        got, comp = check_full(enc, rgb, rt, layers, at, cw, ch, vp, 2, 4, what=(len(layers), at, vp))
        check_full(enc, rgb, rt, layers, at, cw, ch, vp, 2, 4, clear=True, what="clear")
        got, info, _ = check_delta(enc, rgb, None, rt, layers, at, cw, ch, vp, 2, 4, what="no previous composite: the keyframe")
        assert info == dict(keyframe=1, changed=0, emitted=0, runs=0)
        check_delta(enc, rgb, comp, rt, layers, at, cw, ch, vp, 2, 4, clear=True, what="clear_screen: the keyframe")
    # a glyph-only change counts as changed, whatever the tolerance; a resting composite gives the one run at the last cell
    prev = LR.composite(rgb, rt, [wide], 0, cw, ch)
    _, info, comp = check_delta(enc, rgb, prev, rt, [LR.Layer([[ord("z"), ord("y")]], RED, BLUE)], 0, cw, ch, gap=0, tol=255, what="glyph only")
    assert info["changed"] == 1 and info["keyframe"] == 0
    _, info, _ = check_delta(enc, rgb, comp, rt, [LR.Layer([[ord("z"), ord("y")]], RED, BLUE)], 0, cw, ch, gap=8, what="at rest")
    assert info == dict(keyframe=0, changed=0, emitted=1, runs=1)


@FORMS
def test_hook_layers_off_every_edge_outside_and_sixteen(enc, rgb):
    rng = np.random.default_rng(16)
    cw, ch = 23, 9
    rt = random_plane(rng, rgb, 5, 11)
    edges = [(-3, 2), (cw - 2, 3), (4, -2), (5, ch - 1), (-2, -2), (cw - 1, ch - 1), (-4, ch - 2), (cw - 3, -1)]
    layers = [random_layer(rng, 5, 3, x, y) for x, y in edges]
    check_full(enc, rgb, rt, layers, 4, cw, ch, (6, 2), what="off every edge")
    outside = [random_layer(rng, 4, 4, x, y, holes=0) for x, y in [(-4, 0), (cw, 0), (0, -4), (0, ch), (-100, -100), (2 ** 31 - 5, 0), (-2 ** 31, -2 ** 31)]]
    got, _ = check_full(enc, rgb, rt, outside, 3, cw, ch, (6, 2), what="wholly outside")
    S.assert_stream(got, LR.stream(rgb, rt, [], 0, cw, ch, (6, 2)), "layers wholly outside change nothing")
    bigger = [random_layer(rng, cw + 6, ch + 4, -3, -2)]
    check_full(enc, rgb, rt, bigger, 1, cw, ch, (6, 2), what="larger than the console, below")
    check_full(enc, rgb, rt, bigger, 0, cw, ch, (6, 2), what="larger than the console, above")
    check_full(enc, rgb, rt, [random_layer(rng, 1, 1, 22, 8, holes=0)], 0, cw, ch, what="1 x 1 on the last cell")
    sixteen = [random_layer(rng, int(rng.integers(1, 9)), int(rng.integers(1, 5)), int(rng.integers(-3, cw)), int(rng.integers(-2, ch)), holes=0.5) for _ in range(16)]
    for at in (0, 7, 16):
        _, comp = check_full(enc, rgb, rt, sixteen, at, cw, ch, (6, 2), 3, 12, what=("16 layers", at))
    moved = [LR.Layer(l.chars, l.fg, l.bg, l.x + (k % 3) - 1, l.y) for k, l in enumerate(sixteen)]
    check_delta(enc, rgb, comp, rt, moved, 16, cw, ch, (6, 2), 3, 12, gap=2, what="16 layers moved")


@FORMS
def test_hook_mixed_widths_across_lane_and_tile_boundaries(enc, rgb):
    """1027 x 3: width changes fall on the lanes' 4-cell and the tiles' 1024-cell boundaries"""
    rng = np.random.default_rng(1027)
    cw, ch = 1027, 3
    rt = random_plane(rng, rgb, 1, 300)
    layers = [random_layer(rng, cw, ch, 0, 0, holes=0.1)]
    for i, u in [(1020, 0x41), (1021, 0x7FF), (1022, 0x800), (1023, 0x41), (1024, 0xFFFF), (1025, 0x80), (2047, 0x7F), (2048, 0xD800), (3, 0x80), (4, 0x800)]:
        layers[0].chars[i // cw, i % cw] = u
    _, comp = check_full(enc, rgb, rt, layers, 0, cw, ch, (400, 1), what="1027 x 3")
    check_full(enc, rgb, rt, layers, 1, cw, ch, (400, 1), clear=True, what="1027 x 3, below the raytrace framebuffer")
    nxt = [LR.Layer(layers[0].chars.copy(), layers[0].fg, layers[0].bg)]
    for i in (1019, 1023, 1024, 1028, 2047, 2048, 3080):          # glyphs of another width at the boundaries
        nxt[0].chars[i // cw, i % cw] = 0x2580 if nxt[0].chars[i // cw, i % cw] < 0x800 else 0x42
    for gap in (0, 3, 8):
        _, info, _ = check_delta(enc, rgb, comp, rt, nxt, 0, cw, ch, (400, 1), gap=gap, tol=255, what=("1027 x 3", gap))
        assert info["changed"] == 7


@FORMS
@pytest.mark.parametrize("cw,ch,rows", [(3, 11, (8, 9, 10)), (2, 1001, (998, 999, 1000))], ids=["9-10", "999-1000"])
def test_hook_row_numbers_with_layered_cells_in_column_0(enc, rgb, cw, ch, rows):
    rng = np.random.default_rng(ch)
    rt = random_plane(rng, rgb, 4, 2)
    layers = [random_layer(rng, 1, ch, 0, 0, holes=0), random_layer(rng, 1, 2, 0, rows[1], units=np.array([0x800], np.uint16), holes=0)]
    got, comp = check_full(enc, rgb, rt, layers, 1, cw, ch, (1, rows[0] - 1), what=(cw, ch))
    assert all(b"\x1b[%d;1H" % (r + 1) in got for r in rows)
    nxt = [layers[0], LR.Layer(layers[1].chars + 1, layers[1].fg, layers[1].bg, 0, rows[1])]
    got, info, _ = check_delta(enc, rgb, comp, rt, nxt, 1, cw, ch, (1, rows[0] - 1), gap=0, tol=255, what=(cw, ch, "delta"))
    assert info["changed"] == 2 and b"\x1b[%d;1H" % (rows[1] + 1) in got and b"\x1b[%d;1H" % (rows[2] + 1) in got


@FORMS
def test_hook_deltas_outside_and_across_the_raytrace_framebuffers_edge(enc, rgb):
    rng = np.random.default_rng(99)
    cw, ch, vp = 40, 6, (10, 1)
    rt = random_plane(rng, rgb, 4, 20)                                   # columns 10..29, rows 1..4
    base = LR.Layer(np.full((ch, cw), ord("."), np.uint16), GREY, (0.0, 0.0, 0.0))
    prev = LR.composite(rgb, rt, [base], 1, cw, ch, vp)
    # changed cells only outside the raytrace viewport
    out = LR.Layer(base.chars.copy(), base.fg.copy(), base.bg.copy())
    out.chars[0, 5], out.chars[5, 39], out.chars[2, 3] = ord("a"), ord("b"), 0x3A9
    out.chars[2, 15] = ord("c")                                          # (under the raytrace framebuffer: not shown, not changed)
    out.fg[3, 35] = RED
    _, info, _ = check_delta(enc, rgb, prev, rt, [out], 1, cw, ch, vp, gap=0, tol=2, what="outside the viewport")
    assert info["changed"] == 4
    # gap windows across the raytrace framebuffer's edge: a layered cell left of column 10 and a raytrace cell right of it
    for gap in (0, 1, 8):
        for dl, dr in ((1, 0), (1, 1), (2, 3), (5, 4), (1, 8), (9, 0)):
            lay = LR.Layer(base.chars.copy(), base.fg, base.bg)
            lay.chars[2, 10 - dl] = ord("#")
            cur = rt.copy()
            if rgb:
                cur[2 * 1, dr, :3] = cur[2 * 1, dr, :3].astype(np.int64) ^ 0x80
            else:
                cur[1, dr, 0] ^= 0x80
            _, info, _ = check_delta(enc, rgb, prev, cur, [lay], 1, cw, ch, vp, gap=gap, tol=2, what=("across the edge", gap, dl, dr))
            assert info["changed"] == 2 and info["runs"] == (2 if dl + dr - 1 <= gap else 3)          # (the last cell is a run of its own)
    # a resting composite: the one run at the last cell
    _, info, _ = check_delta(enc, rgb, prev, rt, [base], 1, cw, ch, vp, gap=8, what="at rest")
    assert info == dict(keyframe=0, changed=0, emitted=1, runs=1)


def test_hook_24_bit_delta_at_tolerance_0_and_2(enc):
    rng = np.random.default_rng(2)
    cw, ch, vp = 30, 5, (4, 1)
    rt = random_plane(rng, True, 3, 12)
    lay = random_layer(rng, cw, ch, 0, 0, holes=0.3)
    prev = LR.composite(True, rt, [lay], 1, cw, ch, vp)
    cur = rt.copy()
    cur[..., :3] = np.clip(cur[..., :3].astype(np.int64) + rng.integers(-3, 4, cur[..., :3].shape), 0, 255)
    nudged = LR.Layer(lay.chars.copy(), np.clip(lay.fg + rng.uniform(-0.01, 0.01, lay.fg.shape), 0, 1).astype(np.float32), lay.bg)
    nudged.chars[4, 29] = 0x42
    seen = []
    for tol in (0, 2):
        _, info, comp = check_delta(enc, True, prev, cur, [nudged], 1, cw, ch, vp, gap=1, tol=tol, what=("tolerance", tol))
        seen.append(info["changed"])
        # what was not emitted keeps what the terminal shows: chained, the comparison is against that
        check_delta(enc, True, comp, cur, [nudged], 1, cw, ch, vp, gap=1, tol=tol, what=("chained", tol))
    assert seen[0] > seen[1] > 0


@FORMS
def test_hook_random_641x181_with_three_layers(enc, rgb):
    rng = np.random.default_rng(181)
    cw, ch, vp = 641, 181, (1, 0)
    rt = random_plane(rng, rgb, 180, 600)
    rt[:, 100:300] = rt[:, 100:101]                                      # long runs of equal cells too
    layers = [random_layer(rng, cw, ch, 0, 0, holes=0.97), random_layer(rng, 200, 60, 500, 150, holes=0.2), random_layer(rng, 64, 20, -10, -5, holes=0.5)]
    _, comp = check_full(enc, rgb, rt, layers, 1, cw, ch, vp, what="641 x 181")
    cur = rt.copy()
    redraw = rng.random(rt.shape[:2]) < 1 / 8
    cur[redraw] = rng.integers(0, 256, cur[redraw].shape)
    moved = [layers[0], LR.Layer(layers[1].chars, layers[1].fg, layers[1].bg, 497, 149), layers[2]]
    _, info, _ = check_delta(enc, rgb, comp, cur, moved, 1, cw, ch, vp, gap=1, tol=2 if rgb else 0, what="641 x 181, delta")
    assert info["runs"] > 1000 and info["emitted"] > info["changed"]


@FORMS
def test_hook_chained_deltas_leave_the_full_streams_terminal(enc, rgb):
    """a keyframe and then chained deltas into a terminal: cells, cursor and colours are what the full stream leaves (tolerance 0).  Glyphs
    below 0x20 are not drawn here: the terminal model takes none."""
    rng = np.random.default_rng(7)
    cw, ch, vp = 37, 9, (5, 2)
    units = WIDTHS
    screen, prev = LR.Screen(cw, ch), None
    layers = [random_layer(rng, cw, ch, 0, 0, units, 0.6), random_layer(rng, 12, 4, 20, 3, units, 0.2)]
    for k in range(5):
        rt = random_plane(rng, rgb, 5, 24) if k % 2 == 0 else rt
        layers = [layers[0], LR.Layer(layers[1].chars, layers[1].fg, layers[1].bg, 20 - 2 * k, 3 + k % 2)]
        layers[0].chars[8, :] = rng.choice(units, cw)
        got, info, prev = check_delta(enc, rgb, prev, rt, layers, 1, cw, ch, vp, 3, 12, gap=k % 4, what=("chain", k))
        assert info["keyframe"] == int(k == 0)
        screen.feed(got)
        full = LR.stream(rgb, rt, layers, 1, cw, ch, vp, 3, 12)
        assert screen.state() == LR.Screen(cw, ch).feed(full).state(), k


def test_hook_refusals(enc):
    rt = np.zeros((2, 3, 2), np.uint8)
    cap = bound(enc, False, 3, 2)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    fn = enc.L.ycge_test_ansi_layers
    fn.restype, fn.argtypes = abi.ANSI_LAYERS_HOOK_PROTOTYPES["ycge_test_ansi_layers"]
    arr, keep = layer_array([LR.Layer([[65]])])
    call = lambda layers, k, at, gap=1, c=cap: fn(enc.ctx, 0, rt.ctypes.data_as(U8P), 3, 2, layers, k, at, None, None, 3, 2, 0, 0, 7, 0, 0, 1, gap, 0,
                                                 out.ctypes.data_as(U8P), c, C.byref(n), None, None, None)
    for args, words in [((arr, 17, 0), [b"n = 17"]), ((arr, -1, 0), [b"n = -1"]), ((arr, 1, 2), [b"raytrace_at = 2"]), ((arr, 1, -1), [b"raytrace_at = -1"]),
                        ((None, 1, 0), [b"layers is NULL"]), ((arr, 0, 0), [b"n = 0"]), ((arr, 1, 0, 9), [b"merge_gap 9"]),
                        ((arr, 1, 0, 1, cap - 1), [b"capacity %d" % (cap - 1)])]:
        rc = call(*args)
        msg = enc.L.ycge_last_error(enc.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), (args[1:], msg)
    assert not out.any() and n.value == 0
    assert call(arr, 1, 0) == 0 and n.value > 0


# ------------------------------------------------------------------------------------------------------------- 2: the eight stream calls
FBW, FBH, CW, CH, VP = 64, 18, 70, 20, (3, 1)
EXPORTS = [(kind, rgb, delta) for kind in ("frame", "video") for rgb in (False, True) for delta in (False, True)]
EXPORT_IDS = [f"{kind}{'_rgb' if rgb else ''}{'_delta' if delta else ''}" for kind, rgb, delta in EXPORTS]


def console_layers(k, text=None):
    """the reference's arrangement: a console-sized entity framebuffer below the raytrace one, blank but for one text row that changes every
    frame, and a 12 x 4 framebuffer above"""
    chars = np.full((CH, CW), 0x20, np.uint16)
    line = (text or f"frame_{k}_▀_éΩ_{'#' * (k % 5)}").ljust(CW)[:CW]          # (a ' ' is transparent: the default cell shows there)
    chars[CH - 1] = [ord(c) for c in line]
    menu = np.full((4, 12), ord("+"), np.uint16)
    menu[1:3, 1:11] = [ord(c) for c in "menu__" + str(k % 10) + "___"]
    menu[2, 3:6] = 0x20
    return [LR.Layer(chars, WHITE, (0.0, 0.0, 0.5)), LR.Layer(menu, (1.0, 1.0, 0.0), GREY, 50 + k, 2)]


def movie(k):
    rng = np.random.default_rng(3)
    return np.roll(rng.integers(0, 256, (36, 64, 3)).astype(np.uint8), 5 * k, axis=1).copy()


def stream_call(g, v, kind, rgb, delta, k, **kw):
    """one of the eight exports on g's context -> (stream, info or None, SDR array)"""
    r = v if kind == "video" else g
    fn = getattr(r, "TryFlipAndBlitAnsi" + ("Rgb" if rgb else "") + ("Delta" if delta else ""))
    head = (movie(k),) if kind == "video" else ()
    if delta:
        kw.setdefault("merge_gap", 2)
        if rgb:
            kw.setdefault("tolerance", 1)
        stream, info, sdr = fn(*head, CW, CH, VP, 3, 12, sdr=True, **kw)
        return stream, info, sdr
    stream, sdr = fn(*head, CW, CH, VP, 3, 12, sdr=True, **kw)
    return stream, None, sdr


def expected(rgb, delta, prev, sdr, layers, at=1, **kw):
    """the restatement of stream_call: (bytes, info or None, next composite)"""
    plane = LR.frame_plane(rgb, sdr)
    if not delta:
        return LR.stream(rgb, plane, layers, at, CW, CH, VP, 3, 12, kw.get("clear_screen", False)), None, None
    return LR.delta(rgb, prev, plane, layers, at, CW, CH, VP, 3, 12, kw.get("merge_gap", 2), kw.get("tolerance", 1) if rgb else 0, kw.get("clear_screen", False),
                    kw.get("keyframe", False))


def unlayered(rgb, sdr):
    return (R.frame_stream if rgb else A.frame_stream)(sdr, CW, CH, VP, 3, 12)


@pytest.fixture()
def pair(product_lib):
    a, b, pose = S.twins(1, FBW, FBH, 1)
    yield a, b, pose
    a.close(); b.close()


@pytest.mark.parametrize("kind,rgb,delta", EXPORTS, ids=EXPORT_IDS)
def test_each_export_streams_the_layered_console(pair, kind, rgb, delta):
    a, b, pose = pair
    va, vb = VideoRenderer(renderer=a), VideoRenderer(renderer=b)
    prev = None

    def frame(k, layers, keyframe, what):
        """frame k on both contexts - a: the plain call of the same renderer - and b's stream against the restatement"""
        nonlocal prev
        S.move((a, b), pose, k)
        plain = va.TryFlipAndBlit(movie(k), color16=False, sdr=True)["sdr"] if kind == "video" else a.TryFlipAndBlit(want_sdr=True)
        stream, info, sdr = stream_call(b, vb, kind, rgb, delta, k)
        assert pu.bits_equal(plain, sdr), what
        if kind == "frame":
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure, what
        want, winfo, nxt = expected(rgb, delta, None if keyframe else prev, sdr, layers)
        S.assert_stream(stream, want, what)
        if delta:
            assert info == winfo and info["keyframe"] == int(keyframe), (what, info, winfo)
            prev = nxt
        return stream, sdr

    for k in range(3):          # 0 -> n: a keyframe; then set calls that keep n > 0: deltas
        b.SetConsoleLayers(mirror(console_layers(k)), 1)
        stream, _ = frame(k, console_layers(k), k == 0, f"frame {k}")
        assert delta or (("frame_%d_" % k).encode() in stream and ("menu__%d" % k).encode() in stream)
    b.SetConsoleLayers([], 0)          # n -> 0: a keyframe, and the bytes of a context that never had layers
    S.move((a, b), pose, 3)
    s_a = stream_call(a, va, kind, rgb, delta, 3)
    s_b = stream_call(b, vb, kind, rgb, delta, 3)
    S.assert_stream(s_b[0], s_a[0], "n == 0: the bytes of a context that never had layers")
    S.assert_stream(s_b[0], unlayered(rgb, s_b[2]), "n == 0: the unlayered restatement")
    assert pu.bits_equal(s_a[2], s_b[2]) and (not delta or s_b[1]["keyframe"] == 1)
    s_a = stream_call(a, va, kind, rgb, delta, 3)
    s_b = stream_call(b, vb, kind, rgb, delta, 3)
    S.assert_stream(s_b[0], s_a[0], "n == 0: the next stream too")
    assert s_a[1] == s_b[1] and (not delta or s_b[1]["keyframe"] == 0)
    b.SetConsoleLayers(mirror(console_layers(4)), 1)          # 0 -> n again: a keyframe
    prev = None
    frame(4, console_layers(4), True, "0 -> n")
    if kind == "frame":
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))


# ------------------------------------------------------------------------------------------------------------- 3: the state rules
@pytest.fixture()
def one(product_lib):
    a, b, pose = S.twins(1, FBW, FBH, 1)
    a.close()
    yield b, pose
    b.close()


def step(g, prev, layers, rgb=False, keyframe_expected=False, what="", at=1, **kw):
    """one ray-traced delta frame of g, held to the restatement against the composite `prev`; -> the next composite"""
    stream, info, sdr = stream_call(g, None, "frame", rgb, True, 0, **kw)
    want, winfo, nxt = expected(rgb, True, None if keyframe_expected else prev, sdr, layers, at, **kw)
    S.assert_stream(stream, want, what)
    assert info == winfo and info["keyframe"] == int(keyframe_expected), (what, info, winfo)
    return nxt


def test_a_set_call_that_keeps_layers_gives_a_delta_of_the_changed_cells(one):
    g, pose = one
    layers = console_layers(0)
    g.SetConsoleLayers(mirror(layers), 1)
    c = step(g, None, layers, keyframe_expected=True, what="first")
    for k, (layers, at) in enumerate([(console_layers(1), 1), (console_layers(1)[:1], 1), (console_layers(2) + console_layers(7)[1:], 1), (console_layers(2), 2),
                                      (console_layers(2), 0)]):
        g.SetConsoleLayers(mirror(layers), at)          # edited, removed, added, reordered below and above the raytrace framebuffer
        c = step(g, c, layers, at=at, what=f"set call {k}")
    g.SetConsoleLayers(mirror(layers), 0)          # the same layers again, the camera at rest: what changes is the picture's own noise
    step(g, c, layers, at=0, what="the same layers")


def test_a_refused_set_call_leaves_the_layers_in_force(one):
    g, pose = one
    layers = console_layers(0)
    g.SetConsoleLayers(mirror(layers), 1)
    c = step(g, None, layers, keyframe_expected=True)
    arr, keep = layer_array(layers)
    bad_cells = (abi.ConsoleLayer * 1)(abi.ConsoleLayer(0, 0, 2, 2, None))
    bad_size = (abi.ConsoleLayer * 1)(abi.ConsoleLayer(0, 0, 0, 2, arr[0].cells))
    bad_h = (abi.ConsoleLayer * 1)(abi.ConsoleLayer(0, 0, 2, -1, arr[0].cells))
    huge = (abi.ConsoleLayer * 2)(abi.ConsoleLayer(0, 0, 8192, 8192, arr[0].cells), abi.ConsoleLayer(0, 0, 1, 1, arr[0].cells))          # 2^26 + 1 cells: refused unread
    for args, words in [((arr, 17, 0), [b"n = 17"]), ((arr, -1, 0), [b"n = -1"]), ((arr, 2, 3), [b"raytrace_at = 3"]), ((arr, 2, -1), [b"raytrace_at = -1"]),
                        ((None, 2, 0), [b"layers is NULL", b"n = 2"]), ((bad_cells, 1, 0), [b"layers[0].cells is NULL"]), ((bad_size, 1, 0), [b"0 x 2"]),
                        ((bad_h, 1, 0), [b"2 x -1"]), ((huge, 2, 0), [b"2^26"])]:
        rc = g.L.ycge_console_set_layers(g.ctx, *args)
        msg = g.L.ycge_last_error(g.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), (args[1:], msg)
    with pytest.raises(abi.YcgeError):
        g.SetConsoleLayers(mirror(layers), 5)
    c = step(g, c, layers, what="the old layers are in force and the delta state stands")
    g.SetConsoleLayers(mirror(layers[:1]), 0)
    step(g, c, layers[:1], at=0, what="usable")


def test_a_peer_context_is_refused(product_lib):
    a, b, pose = S.twins(2, 160, 45, 1, devices=[0, 0, 0])
    try:
        fn = b.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int32]
        peer = fn(b.ctx, 0)
        assert peer
        arr, keep = layer_array(console_layers(0))
        assert b.L.ycge_console_set_layers(peer, arr, 2, 1) == abi.YCGE_ERR_INVALID_ARG and b"driven by their root" in b.L.ycge_last_error(peer)
    finally:
        a.close(); b.close()


@FORMS
def test_resize_and_scene_upload_keep_the_layers_and_resize_keyframes(one, rgb):
    g, pose = one
    layers = console_layers(0)
    g.SetConsoleLayers(mirror(layers), 1)
    c = step(g, None, layers, rgb, keyframe_expected=True)
    c = step(g, c, layers, rgb, what="delta")
    g.Resize(48, 12, 1)
    c = step(g, c, layers, rgb, keyframe_expected=True, what="after Resize: a keyframe, the layers kept")
    c = step(g, c, layers, rgb, what="delta at the new size")
    g.UploadScene(g.flat)
    c = step(g, c, layers, rgb, what="a scene upload keeps the layers and the delta state")
    g.TryFlipAndBlitAnsiRgb(CW, CH, VP, 3, 12) if rgb else g.TryFlipAndBlitAnsi(CW, CH, VP, 3, 12)
    c = step(g, c, layers, rgb, keyframe_expected=True, what="after a full stream")
    step(g, c, layers, not rgb, keyframe_expected=True, what="the other colour form")


@FORMS
def test_a_video_delta_follows_a_ray_traced_one_on_the_shared_context(one, rgb):
    g, pose = one
    v = VideoRenderer(renderer=g)
    layers = console_layers(0)
    v.SetConsoleLayers(mirror(layers), 1)          # (the same context: either renderer sets them)
    kw = dict(tolerance=0) if rgb else {}
    c = step(g, None, layers, rgb, keyframe_expected=True, **kw)
    stream, info, sdr = stream_call(g, v, "video", rgb, True, 1, **kw)
    want, winfo, c = expected(rgb, True, c, sdr, layers, **kw)
    S.assert_stream(stream, want, "video against the ray-traced frame")
    assert info == winfo and info["keyframe"] == 0 and info["changed"] > 0
    g.SetConsoleLayers(mirror(console_layers(1)), 1)
    stream, info, sdr = stream_call(g, v, "video", rgb, True, 1, **kw)
    want, winfo, c = expected(rgb, True, c, sdr, console_layers(1), **kw)
    S.assert_stream(stream, want, "the same picture, another text row")
    assert info == winfo and 0 < info["changed"] < 2 * CW          # (the text row's and the moved menu's cells alone)
    step(g, c, console_layers(1), rgb, what="ray-traced against the video frame", **kw)
