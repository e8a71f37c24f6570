"""The layered ANSI streams restated in plain Python - what the eight stream calls return once ycge_console_set_layers has named the
console's other framebuffers, and what ycge_test_ansi_layers returns - in both colour forms.

The composite is ansi_stream_restatement.Renderer's: GetChexelForPoint (ANSITerminalRenderer.cs:67-84) over the list of framebuffers,
bottom first, taken literally - the topmost framebuffer whose chexel at the point has Char != ' ' wins, else the default cell.  The full
256-colour stream is that Renderer's Render() line for line, with AppendCharUtf8 (:204-224) restated on the UTF-16 code unit (a lone
surrogate has a 3-byte form there that Python's encoder refuses).  The 24-bit stream and the two deltas generalise ansi_rgb_restatement
and ansi_delta_restatement to console-wide (char, fg, bg) cells: a cell changed when its character differs from the previous composite's
or its colours do (256 colours: either index; 24-bit: the largest channel difference exceeds the tolerance).

A layer's colours are encoded by the encoder the frames use (chexel_restatement): ansi256 of the float colour, or its sRGB8 triple.
"""
from __future__ import annotations

import numpy as np

import ansi_delta_restatement as D
import ansi_rgb_restatement as R
import ansi_stream_restatement as A
import chexel_restatement as CR

INFO = D.INFO
BLOCK = 0x2580


class Layer:
    """One of the console's other framebuffers: chars (h, w) UTF-16 code units, fg / bg (h, w, 3) float32 (one colour broadcasts), at (x, y)."""

    def __init__(self, chars, fg=(0.75, 0.75, 0.75), bg=(0.0, 0.0, 0.0), x=0, y=0):
        self.chars = np.array(chars, dtype=np.uint16)
        assert self.chars.ndim == 2 and self.chars.size > 0
        self.h, self.w = self.chars.shape
        self.fg = np.array(np.broadcast_to(np.asarray(fg, np.float32), (self.h, self.w, 3)))          # (copies: a test may edit a cell)
        self.bg = np.array(np.broadcast_to(np.asarray(bg, np.float32), (self.h, self.w, 3)))
        self.x, self.y = int(x), int(y)


def utf8(unit: int) -> bytes:
    """AppendCharUtf8 (:204-224) on a UTF-16 code unit"""
    if unit <= 0x7F:
        return bytes([unit])
    if unit <= 0x7FF:
        return bytes([0xC0 | (unit >> 6), 0x80 | (unit & 0x3F)])
    return bytes([0xE0 | (unit >> 12), 0x80 | ((unit >> 6) & 0x3F), 0x80 | (unit & 0x3F)])


class _Framebuffer(A.Framebuffer):
    """A.Framebuffer whose colours may be triples: fg / bg (h, w) indices or (h, w, 3) sRGB8"""

    def __init__(self, chars, fg, bg, vx=0, vy=0):
        self.chars, self.fg, self.bg = chars, np.asarray(fg), np.asarray(bg)
        self.Height, self.Width = self.fg.shape[:2]
        self.ViewportX, self.ViewportY = vx, vy

    def GetChexel(self, x, y):
        f, b = self.fg[y, x], self.bg[y, x]
        if f.ndim == 0:
            return self.chars[y][x], int(f), int(b)
        return self.chars[y][x], tuple(int(v) for v in f), tuple(int(v) for v in b)


class Renderer(A.Renderer):
    """A.Renderer with AppendCharUtf8 on the code unit, and in 24-bit colour the default cell's triples"""

    def __init__(self, frame_buffers, default_fg, default_bg, rgb=False):
        super().__init__(frame_buffers, default_fg, default_bg)
        if rgb:
            pal = R.palette_rgb()
            self.default_cell = (" ", pal[default_fg], pal[default_bg])

    def AppendCharUtf8(self, ch: str):
        self.out += utf8(ord(ch))


def _chars(units):
    return [[chr(int(u)) for u in row] for row in np.asarray(units)]


def renderer(rgb, plane, layers, raytrace_at, viewport=(0, 0), default_fg=7, default_bg=0) -> Renderer:
    """the console's frameBuffers list: layers[:raytrace_at], the raytrace framebuffer over `plane` (rgb: the (2 fbH, fbW, 4) RGBA plane, else
    the (fbH, fbW, 2) pairs; every chexel '▀') at `viewport`, layers[raytrace_at:]"""
    plane = np.asarray(plane)
    assert 0 <= raytrace_at <= len(layers)
    if rgb:
        fbH, fbW = plane.shape[0] // 2, plane.shape[1]
        rfg, rbg = plane[0::2, :, :3], plane[1::2, :, :3]
    else:
        fbH, fbW = plane.shape[:2]
        rfg, rbg = plane[..., 0], plane[..., 1]
    fbs = []
    for l in layers:
        if rgb:
            fg, bg = (CR.srgb8_v(CR._clamp01_v(c).astype(np.float64)) for c in (l.fg, l.bg))
        else:
            fg, bg = CR.ansi256_v(l.fg), CR.ansi256_v(l.bg)
        fbs.append(_Framebuffer(_chars(l.chars), fg, bg, l.x, l.y))
    fbs.insert(raytrace_at, _Framebuffer([[A.UPPER_HALF] * fbW for _ in range(fbH)], rfg, rbg, viewport[0], viewport[1]))
    return Renderer(fbs, default_fg, default_bg, rgb)


def composite(rgb, plane, layers, raytrace_at, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0):
    """(glyphs (ch, cw) uint16, colours): GetChexelForPoint at every console cell.  colours: 256 colours (ch, cw, 2) uint8 {fg, bg}; 24-bit the
    (2 ch, cw, 4) RGBA plane of a console-sized framebuffer, the fourth byte 255 - the forms the hook takes and returns"""
    r = renderer(rgb, plane, layers, raytrace_at, viewport, default_fg, default_bg)
    glyphs = np.zeros((console_h, console_w), np.uint16)
    colours = np.full((2 * console_h, console_w, 4), 255, np.uint8) if rgb else np.zeros((console_h, console_w, 2), np.uint8)
    for y in range(console_h):
        for x in range(console_w):
            ch, fg, bg = r.GetChexelForPoint(x, y)
            glyphs[y, x] = ord(ch)
            if rgb:
                colours[2 * y, x, :3], colours[2 * y + 1, x, :3] = fg, bg
            else:
                colours[y, x] = (fg, bg)
    return glyphs, colours


def _cells(rgb, colours):
    """a composite's colours as rows of fg and of bg values: indices, or triples"""
    if rgb:
        return R._triples(colours[0::2, :, :3].astype(np.int64)), R._triples(colours[1::2, :, :3].astype(np.int64))
    return colours[..., 0].astype(np.int64).tolist(), colours[..., 1].astype(np.int64).tolist()


def stream_of(rgb, glyphs, colours, clear=False) -> bytes:
    """Render() (:86-153) over a composite: the walk of ansi_stream_restatement.Renderer.Render, the escapes by the two _sgr helpers"""
    sgr, none = (R._sgr, None) if rgb else (D._sgr, -1)
    fg, bg = _cells(rgb, colours)
    console_h, console_w = glyphs.shape
    out = bytearray(b"\x1b[2J\x1b[H" if clear else b"")
    cur_fg = cur_bg = none
    for y in range(console_h):
        out += b"\x1b[%d;1H" % (y + 1)
        for x in range(console_w):
            out += sgr(fg[y][x], bg[y][x], cur_fg, cur_bg)
            cur_fg, cur_bg = fg[y][x], bg[y][x]
            out += utf8(int(glyphs[y, x]))
    out += b"\x1b[0m"
    return bytes(out)


def stream(rgb, plane, layers, raytrace_at, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, clear=False) -> bytes:
    """the full stream of the layered console.  256 colours: Renderer.Render() itself, line for line; 24-bit: the same walk on triples"""
    if not rgb:
        return renderer(False, plane, layers, raytrace_at, viewport, default_fg, default_bg).Render(console_w, console_h, clear)
    return stream_of(True, *composite(True, plane, layers, raytrace_at, console_w, console_h, viewport, default_fg, default_bg), clear)


def bound(rgb, console_w, console_h) -> int:
    return (R.bound if rgb else A.bound)(console_w, console_h)


def delta_of(rgb, prev, cur, gap=1, tol=0, clear=False, keyframe=False):
    """(bytes, info, next composite) of the stream that follows a terminal showing the composite `prev` = (glyphs, colours), or None, with the
    composite `cur`.  The next composite: cur's glyphs; cur's colours, and in 24-bit colour cur's where a cell was emitted and prev's elsewhere"""
    glyphs, colours = cur
    if prev is None or clear or keyframe:
        return stream_of(rgb, glyphs, colours, clear), dict(zip(INFO, (1, 0, 0, 0))), (glyphs.copy(), colours.copy())
    pglyphs, pcolours = prev
    assert pglyphs.shape == glyphs.shape and pcolours.shape == colours.shape and 0 <= gap <= 8 and 0 <= tol <= 255
    if rgb:
        d = np.abs(colours[..., :3].astype(np.int64) - pcolours[..., :3].astype(np.int64)).max(axis=-1)          # (2 ch, cw)
        differs = np.maximum(d[0::2], d[1::2]) > tol
    else:
        differs = (colours != pcolours).any(axis=-1)
    changed = differs | (glyphs != pglyphs)
    em = D.emitted_mask(changed, gap)
    sgr, none = (R._sgr, None) if rgb else (D._sgr, -1)
    fg, bg = _cells(rgb, colours)
    out = bytearray()
    runs = 0
    for y, x in np.argwhere(em):                               # (raster order)
        y, x = int(y), int(x)
        if x == 0 or not em[y, x - 1]:
            out += b"\x1b[%d;%dH" % (y + 1, x + 1)
            out += sgr(fg[y][x], bg[y][x], none, none)
            runs += 1
        else:
            out += sgr(fg[y][x], bg[y][x], fg[y][x - 1], bg[y][x - 1])
        out += utf8(int(glyphs[y, x]))
    out += b"\x1b[0m"
    if rgb:
        nxt = pcolours.copy()
        nxt[..., 3] = 255
        both = np.repeat(em, 2, axis=0)
        nxt[both] = colours[both]
    else:
        nxt = colours.copy()
    return bytes(out), dict(zip(INFO, (0, int(changed.sum()), int(em.sum()), runs))), (glyphs.copy(), nxt)


def delta(rgb, prev, plane, layers, raytrace_at, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, gap=1, tol=0, clear=False,
          keyframe=False):
    """delta_of for the layered console over `plane`"""
    cur = composite(rgb, plane, layers, raytrace_at, console_w, console_h, viewport, default_fg, default_bg)
    return delta_of(rgb, prev, cur, gap, tol, clear, keyframe)


def frame_plane(rgb, sdr):
    """the framebuffer plane of a frame whose SDR array (fbH, fbW, 2, 3) is given"""
    return R.frame_rgba(sdr) if rgb else CR.encode(sdr)[1]


class Screen(R.Screen):
    """A terminal for these streams: the tokens of either colour form, and as a character any 1-, 2- or 3-byte UTF-8 form of a code unit
    of 0x20 and above (a lone surrogate's included).  grid[y][x] = (code unit, fg, bg); the colours are indices or triples."""

    def feed(self, s: bytes):
        i = 0
        while i < len(s):
            b = s[i]
            if b == 0x1B:
                j = self._escape(s, i)
            elif 0x20 <= b < 0x80:
                self._put(b); j = i + 1
            elif 0xC0 <= b < 0xE0:
                assert i + 1 < len(s) and s[i + 1] & 0xC0 == 0x80, ("a 2-byte form cut short", i)
                self._put((b & 0x1F) << 6 | (s[i + 1] & 0x3F)); j = i + 2
            elif 0xE0 <= b < 0xF0:
                assert i + 2 < len(s) and s[i + 1] & 0xC0 == 0x80 and s[i + 2] & 0xC0 == 0x80, ("a 3-byte form cut short", i)
                self._put((b & 0x0F) << 12 | (s[i + 1] & 0x3F) << 6 | (s[i + 2] & 0x3F)); j = i + 3
            else:
                raise AssertionError(("a byte no stream contains", i, s[max(0, i - 12):i + 12]))
            i = j
        return self

    def _escape(self, s: bytes, i: int) -> int:
        if s[i:i + 4] == b"\x1b[2J":
            self.grid = [[(0x20, None, None)] * self.w for _ in range(self.h)]
            return i + 4
        if s[i:i + 3] == b"\x1b[H":
            self.cursor = (0, 0, False)
            return i + 3
        if s[i:i + 4] == b"\x1b[0m":
            self.colours = (None, None)
            return i + 4
        head = s[i:i + 7]
        if head in (b"\x1b[38;5;", b"\x1b[48;5;", b"\x1b[38;2;", b"\x1b[48;2;"):
            first_is_fg, number = head[2:4] == b"38", (self._triple if head[5:6] == b"2" else self._index)
            v, i = number(s, i + 7)
            if first_is_fg and s[i:i + 6] == b";48;" + head[5:6] + b";":
                b, i = number(s, i + 6)
                self.colours = (v, b)
            else:
                self.colours = (v, self.colours[1]) if first_is_fg else (self.colours[0], v)
            assert s[i:i + 1] == b"m", ("SGR without its m", i)
            return i + 1
        assert s[i:i + 2] == b"\x1b[", ("an escape no stream contains", i)
        r, i = self._number(s, i + 2)
        assert s[i:i + 1] == b";", ("a cursor move without its column", i)
        c, i = self._number(s, i + 1)
        assert s[i:i + 1] == b"H" and 1 <= r <= self.h and 1 <= c <= self.w, ("cursor move", r, c, i)
        self.cursor = (r - 1, c - 1, False)
        return i + 1

    def _index(self, s: bytes, i: int):
        v, i = self._number(s, i)
        assert v <= 255
        return v, i
