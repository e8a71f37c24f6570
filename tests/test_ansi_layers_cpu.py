"""The layered ANSI streams without a GPU: the restatement (tests/ansi_layers_restatement.py) held to hand-written bytes on 1 x 1 and 2 x 1
consoles - the UTF-8 widths, transparency, the order of the framebuffers, what counts as changed - and to the two bounds; and the
declarations of ycge_console_set_layers and its hook in every mirror."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import ansi_layers_restatement as LR
import ansi_rgb_restatement as R
import ansi_stream_restatement as A
import chexel_restatement as CR
from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXPORT = "ycge_console_set_layers"
HOOK = "ycge_test_ansi_layers"
RED, BLUE, WHITE = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0)
PAL = A.default_indices()          # ansi(palette16[k])
BLOCK = "▀".encode("utf-8")


def idx(c):
    return CR.ansi256(np.asarray(c, np.float32))


def rgb8(c):
    return tuple(int(v) for v in CR.srgb8_v(np.asarray(c, np.float64)))


def pairs(*cells):
    """one framebuffer row of {fg, bg} pairs"""
    return np.array([list(cells)], np.uint8)


def plane(*cells):
    """one framebuffer row of {fg triple, bg triple} as an RGBA plane"""
    p = np.full((2, len(cells), 4), 255, np.uint8)
    for x, (f, b) in enumerate(cells):
        p[0, x, :3], p[1, x, :3] = f, b
    return p


def both(f, b):
    return b"\x1b[38;5;%d;48;5;%dm" % (f, b)


def both_rgb(f, b):
    return b"\x1b[38;2;%d;%d;%d;48;2;%d;%d;%dm" % (f + b)


def one(unit, fg=RED, bg=BLUE, x=0, y=0):
    return LR.Layer([[unit]], fg, bg, x, y)


# ------------------------------------------------------------------------------------------------------------- the character
def test_utf8_is_appendcharutf8_on_the_code_unit():
    assert LR.utf8(0x7F) == b"\x7f" and LR.utf8(0x80) == b"\xc2\x80"
    assert LR.utf8(0x7FF) == b"\xdf\xbf" and LR.utf8(0x800) == b"\xe0\xa0\x80"
    assert LR.utf8(0xD800) == b"\xed\xa0\x80" and LR.utf8(0xDFFF) == b"\xed\xbf\xbf"          # a lone surrogate: its 3-byte form
    assert LR.utf8(0xFFFF) == b"\xef\xbf\xbf" and LR.utf8(0) == b"\x00" and LR.utf8(0x2580) == BLOCK
    for u in (0x20, 0x41, 0xE9, 0x3A9, 0x20AC, 0x2580, 0xFFFD):
        assert LR.utf8(u) == chr(u).encode("utf-8"), hex(u)


def test_the_three_widths_on_a_one_cell_console():
    for unit in (0x00, 0x7F, 0x80, 0x7FF, 0x800, 0xD800, 0xFFFF):
        want = b"\x1b[1;1H" + both(idx(RED), idx(BLUE)) + LR.utf8(unit) + b"\x1b[0m"
        for at in (0, 1):          # below the raytrace framebuffer it shows where that does not reach: here the framebuffer lies off the console
            assert LR.stream(False, pairs((1, 2)), [one(unit)], at, 1, 1, viewport=(5, 5)) == want, (hex(unit), at)
        assert LR.stream(False, pairs((1, 2)), [one(unit)], 0, 1, 1) == want, "a layer above the raytrace framebuffer covers it"
        want = b"\x1b[1;1H" + both_rgb(rgb8(RED), rgb8(BLUE)) + LR.utf8(unit) + b"\x1b[0m"
        assert LR.stream(True, plane(((1, 2, 3), (4, 5, 6))), [one(unit)], 0, 1, 1) == want, hex(unit)


def test_a_space_is_transparent_whatever_its_colours():
    # a ' ' with a red background over the raytrace chexel: the chexel shows; over nothing: the default cell, not the red
    lay = [one(0x20, WHITE, RED)]
    assert LR.stream(False, pairs((9, 10)), lay, 0, 1, 1) == b"\x1b[1;1H" + both(9, 10) + BLOCK + b"\x1b[0m"
    assert LR.stream(False, pairs((9, 10)), lay, 0, 1, 1, viewport=(3, 0), default_fg=2, default_bg=4) == b"\x1b[1;1H" + both(PAL[2], PAL[4]) + b" \x1b[0m"
    pal = R.palette_rgb()
    assert LR.stream(True, plane(((9, 9, 9), (1, 1, 1))), lay, 0, 1, 1, viewport=(3, 0), default_fg=2, default_bg=4) == \
        b"\x1b[1;1H" + both_rgb(pal[2], pal[4]) + b" \x1b[0m"
    # ch == 0 is a character
    assert LR.stream(False, pairs((9, 10)), [one(0, WHITE, RED)], 0, 1, 1) == b"\x1b[1;1H" + both(idx(WHITE), idx(RED)) + b"\x00\x1b[0m"


def test_topmost_wins_and_a_space_falls_through():
    a, b, hole = one(ord("a"), RED, BLUE), one(ord("b"), BLUE, RED), one(0x20, WHITE, WHITE)
    rt = pairs((9, 10))
    cell = lambda f, bg, ch: b"\x1b[1;1H" + both(f, bg) + ch + b"\x1b[0m"
    assert LR.stream(False, rt, [a, b], 0, 1, 1) == cell(idx(BLUE), idx(RED), b"b")
    assert LR.stream(False, rt, [b, a], 0, 1, 1) == cell(idx(RED), idx(BLUE), b"a")
    assert LR.stream(False, rt, [a, hole], 0, 1, 1) == cell(idx(RED), idx(BLUE), b"a")            # through the hole to the layer below
    assert LR.stream(False, rt, [a, hole], 1, 1, 1) == cell(9, 10, BLOCK)                          # ... to the raytrace chexel between them
    assert LR.stream(False, rt, [a, b], 2, 1, 1) == cell(9, 10, BLOCK)                             # both below the raytrace framebuffer
    assert LR.stream(False, rt, [hole, hole], 1, 1, 1, viewport=(1, 0)) == cell(PAL[7], PAL[0], b" ")


def test_a_layer_below_the_raytrace_framebuffer_shows_only_outside_it():
    under = LR.Layer([[ord("x"), ord("y")]], RED, BLUE)
    rt = pairs((9, 10))
    want = b"\x1b[1;1H" + both(9, 10) + BLOCK + both(idx(RED), idx(BLUE)) + b"y\x1b[0m"
    assert LR.stream(False, rt, [under], 1, 2, 1) == want
    want = b"\x1b[1;1H" + both(idx(RED), idx(BLUE)) + b"x" + both(9, 10) + BLOCK + b"\x1b[0m"
    assert LR.stream(False, rt, [under], 1, 2, 1, viewport=(1, 0)) == want
    assert LR.stream(False, rt, [under], 0, 2, 1) == b"\x1b[1;1H" + both(idx(RED), idx(BLUE)) + b"xy\x1b[0m"          # above it: both cells


def test_a_glyph_only_change_counts_as_changed():
    rt = pairs((9, 10))
    for rgb, p in ((False, rt), (True, plane(((9, 9, 9), (1, 1, 1))))):
        prev = LR.composite(rgb, p, [LR.Layer([[ord("x"), ord("y")]], RED, BLUE)], 0, 2, 1)
        got, info, nxt = LR.delta(rgb, prev, p, [LR.Layer([[ord("z"), ord("y")]], RED, BLUE)], 0, 2, 1, gap=0, tol=255)
        f, b = (rgb8(RED), rgb8(BLUE)) if rgb else (idx(RED), idx(BLUE))
        esc = both_rgb(f, b) if rgb else both(f, b)
        assert info == dict(keyframe=0, changed=1, emitted=2, runs=1), (rgb, info)          # the changed cell, and the console's last cell behind it
        assert got == b"\x1b[1;1H" + esc + b"zy\x1b[0m"
        assert nxt[0].tolist() == [[ord("z"), ord("y")]]
        # a resting composite: the one run at the last cell
        got, info, _ = LR.delta(rgb, nxt, p, [LR.Layer([[ord("z"), ord("y")]], RED, BLUE)], 0, 2, 1, gap=8)
        assert info == dict(keyframe=0, changed=0, emitted=1, runs=1) and got == b"\x1b[1;2H" + esc + b"y\x1b[0m"
    # 256 colours: a colour-only change in either index
    prev = LR.composite(False, rt, [one(ord("x"))], 0, 1, 1)
    assert LR.delta(False, prev, rt, [one(ord("x"), RED, WHITE)], 0, 1, 1)[1]["changed"] == 1
    # 24-bit: under the tolerance a colour change alone is none, a glyph change still is
    prev = LR.composite(True, plane(((100, 100, 100), (0, 0, 0))), [], 0, 1, 1)
    assert LR.delta(True, prev, plane(((102, 100, 100), (0, 0, 0))), [], 0, 1, 1, tol=2)[1]["changed"] == 0
    assert LR.delta(True, prev, plane(((102, 100, 100), (0, 0, 0))), [one(ord("x"))], 0, 1, 1, tol=255)[1]["changed"] == 1


def test_the_full_stream_is_render_line_for_line():
    """with no layers the restatement is ansi_stream_restatement's own; the generalised walk agrees with Render() on a layered console"""
    rng = np.random.default_rng(1)
    p = rng.integers(0, 256, (3, 5, 2)).astype(np.uint8)
    assert LR.stream(False, p, [], 0, 7, 4, (1, 1), 3, 12, True) == A.stream(p, 7, 4, (1, 1), 3, 12, True)
    q = rng.integers(0, 256, (6, 5, 4)).astype(np.uint8)
    assert LR.stream(True, q, [], 0, 7, 4, (1, 1), 3, 12, True) == R.stream(q, 7, 4, (1, 1), 3, 12, True)
    lay = [random_layer(rng, 7, 4), random_layer(rng, 7, 4)]
    assert LR.stream(False, p, lay, 1, 7, 4, (1, 1), 3, 12) == LR.stream_of(False, *LR.composite(False, p, lay, 1, 7, 4, (1, 1), 3, 12))


def random_layer(rng, cw, ch, units=(0x20, 0x20, 0x41, 0x7F, 0x80, 0x7FF, 0x800, 0x2580, 0xD800, 0xFFFF, 0)):
    """a layer that may hang off any edge of a cw x ch console: a third of its cells transparent, the glyphs of every width"""
    w, h = int(rng.integers(1, cw + 3)), int(rng.integers(1, ch + 3))
    chars = rng.choice(np.array(units, np.uint16), (h, w))
    return LR.Layer(chars, rng.random((h, w, 3)).astype(np.float32), rng.random((h, w, 3)).astype(np.float32),
                    int(rng.integers(-w, cw + 1)), int(rng.integers(-h, ch + 1)))


def test_random_layered_streams_stay_within_the_two_bounds_and_leave_the_full_streams_terminal():
    rng = np.random.default_rng(26)
    for case in range(24):
        rgb = bool(case % 2)
        cw, ch = int(rng.integers(1, 12)), int(rng.integers(1, 6))
        fbW, fbH = int(rng.integers(1, 10)), int(rng.integers(1, 5))
        vp = (int(rng.integers(-3, 5)), int(rng.integers(-2, 3)))
        screen, prev = LR.Screen(cw, ch), None
        for k in range(4):
            p = rng.integers(0, 256, (2 * fbH, fbW, 4) if rgb else (fbH, fbW, 2)).astype(np.uint8)
            lay = [random_layer(rng, cw, ch, units=(0x20, 0x41, 0x7F, 0x80, 0x7FF, 0x800, 0x2580, 0xD800, 0xFFFF)) for _ in range(int(rng.integers(0, 4)))]
            at = int(rng.integers(0, len(lay) + 1))
            full = LR.stream(rgb, p, lay, at, cw, ch, vp, 3, 12, clear=True)
            assert len(full) <= LR.bound(rgb, cw, ch), (case, k)
            got, info, prev = LR.delta(rgb, prev, p, lay, at, cw, ch, vp, 3, 12, gap=int(rng.integers(0, 9)))
            assert len(got) <= LR.bound(rgb, cw, ch) - (0 if k == 0 else 7) and info["keyframe"] == int(k == 0), (case, k)
            screen.feed(got)
            assert screen.state() == LR.Screen(cw, ch).feed(LR.stream(rgb, p, lay, at, cw, ch, vp, 3, 12)).state(), (case, k)


def test_the_widest_character_is_the_block():
    # every cell a 3-byte glyph and every escape at its longest: the bound is reached, never passed
    lay = [LR.Layer(np.full((1, 2), 0xFFFF, np.uint16), np.array([[WHITE, (0.99, 1.0, 1.0)]], np.float32), np.array([[WHITE, (1.0, 1.0, 0.99)]], np.float32))]
    got = LR.stream(True, plane(((0, 0, 0), (0, 0, 0))), lay, 0, 2, 1, clear=True)
    assert len(got) == R.bound(2, 1)


# ------------------------------------------------------------------------------------------------------------- declarations
def test_the_export_and_the_hook_are_declared_in_every_mirror(product_lib):
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    assert re.search(r"\bint " + EXPORT + r"\(ycge_ctx \*ctx, const ycge_console_layer \*layers, int32_t n, int32_t raytrace_at\);", header)
    assert not re.search(r"\b" + EXPORT + r"\s*\(", hooks)
    assert EXPORT in abi.EXPORTED_SYMBOLS and hasattr(product_lib, EXPORT)
    assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int " + EXPORT + r"\(IntPtr ctx, YConsoleLayer\* layers, int n, int raytraceAt\);", cs)
    assert list(abi.ANSI_LAYERS_HOOK_PROTOTYPES) == [HOOK] and HOOK not in abi.EXPORTED_SYMBOLS
    assert re.search(r"\bint " + HOOK + r"\(", hooks) and HOOK not in header and hasattr(product_lib, HOOK)
    n_args = len(re.search(r"\bint " + HOOK + r"\(([^;]*)\);", hooks).group(1).split(","))
    assert n_args == len(abi.ANSI_LAYERS_HOOK_PROTOTYPES[HOOK][1]) == 26
    assert "#define YCGE_ABI_VERSION 10" in header and "#define YCGE_CONSOLE_MAX_LAYERS 16" in header and abi.CONSOLE_MAX_LAYERS == 16
    assert "typedef struct ycge_chexel { uint16_t ch; uint16_t pad; float fg[3]; float bg[3]; } ycge_chexel;" in header
    assert "typedef struct ycge_console_layer { int32_t x, y, w, h; const ycge_chexel *cells; } ycge_console_layer;" in header


def test_the_struct_mirrors_have_the_c_layout():
    from yetanotherconsolegameengine_amd import renderer
    assert C.sizeof(abi.Chexel) == 28 and abi.Chexel.fg.offset == 4 and abi.Chexel.bg.offset == 16
    assert renderer.CHEXEL_DTYPE.itemsize == 28 and [renderer.CHEXEL_DTYPE.fields[f][1] for f in ("ch", "pad", "fg", "bg")] == [0, 2, 4, 16]
    assert C.sizeof(abi.ConsoleLayer) == 24 and abi.ConsoleLayer.cells.offset == 16
    cs = (ROOT / "bindings" / "csharp" / "YcgeConsole.cs").read_text()
    assert re.search(r"public struct YChexel\s*//[^\n]*\n\s*\{\s*public ushort Ch;[^\n]*\n\s*public ushort Pad;\s*public YVec3 Fg;[^\n]*\n\s*public YVec3 Bg;", cs)
    assert re.search(r"public unsafe struct YConsoleLayer[^{]*\{\s*public int X, Y, W, H;[^\n]*\n\s*public YChexel\* Cells;", cs)
    l = renderer.ConsoleLayer(["ab", "c "], RED, BLUE, x=3, y=-1)
    cells = l.cells()
    assert cells["ch"].tolist() == [97, 98, 99, 32] and cells["fg"][2].tolist() == list(RED) and cells["bg"][0].tolist() == list(BLUE)
    s = l.as_struct()
    assert (s.x, s.y, s.w, s.h) == (3, -1, 2, 2) and s.cells[1].ch == 98 and s.cells[3].bg[2] == 1.0


def test_the_export_and_the_hook_sit_behind_the_exception_barrier():
    csrc = Path(abi.__file__).resolve().parent / "csrc"
    text = (csrc / "ycge_ansi.cpp").read_text()
    for n in (EXPORT, HOOK):
        assert re.search(r"^int " + n + r"\([^{;]*?\)\ntry \{\n(.*?)\n\}\ncatch \(\.\.\.\) \{ return ycge_host::abi_catch\(", text, re.S | re.M), n


def test_the_wrappers_send_the_presenters_other_framebuffers():
    cs = ROOT / "bindings" / "csharp"
    presenter = (cs / "HipRaytraceWrapper.cs").read_text()
    assert re.search(r"public void AddFrameBuffer\(Framebuffer fb\) \{ FrameBuffers\.Add\(fb\); \}", presenter)
    assert re.search(r"public void RemoveFrameBuffer\(Framebuffer fb\) \{ FrameBuffers\.Remove\(fb\); \}", presenter)
    for fname in ("HipRaytraceWrapper.cs", "HipVideoWrapper.cs"):
        text = (cs / fname).read_text()
        at = text.index("HipConsoleLayers.Set(ctx, ansi.FrameBuffers, fb);")
        assert at < text.index("Ycge.Check(ctx, Ycge.ycge_" + ("render_frame" if "Raytrace" in fname else "video_blit") + "_ansi_rgb_delta(", at), fname
    assert "Ycge.ycge_console_set_layers(ctx, l, others.Count, raytraceAt)" in (cs / "YcgeConsole.cs").read_text()


def test_a_null_context_is_refused(product_lib):
    cell = abi.Chexel(ord("x"), 0, (C.c_float * 3)(*RED), (C.c_float * 3)(*BLUE))
    layer = (abi.ConsoleLayer * 1)(abi.ConsoleLayer(0, 0, 1, 1, C.pointer(cell)))
    assert product_lib.ycge_console_set_layers(None, layer, 1, 0) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_console_set_layers(None, None, 0, 0) == abi.YCGE_ERR_INVALID_ARG
    fn = product_lib.ycge_test_ansi_layers
    fn.restype, fn.argtypes = abi.ANSI_LAYERS_HOOK_PROTOTYPES[HOOK]
    out, n = np.zeros(64, np.uint8), C.c_size_t(0)
    p = np.zeros(2, np.uint8)
    U8P = C.POINTER(C.c_uint8)
    assert fn(None, 0, p.ctypes.data_as(U8P), 1, 1, layer, 1, 0, None, None, 1, 1, 0, 0, 7, 0, 0, 0, 0, 0, out.ctypes.data_as(U8P), 64, C.byref(n), None, None,
              None) == abi.YCGE_ERR_INVALID_ARG
    assert not out.any() and n.value == 0
