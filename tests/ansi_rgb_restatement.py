"""The 24-bit colour ANSI streams restated in plain Python, from the contract in include/ycge.h alone - what ycge_render_frame_ansi_rgb,
ycge_render_frame_ansi_rgb_delta, the two video calls and the two hooks return - and a terminal model for them.

The reference has no 24-bit presenter: the rules are ANSITerminalRenderer.Render()'s (:86-153) with an sRGB8 triple where it has a
palette index.  A colour image is the RGBA plane of ycge_render_frame_chexels: (2 fbH, fbW, 4) uint8, row 2 cy the top half-cell of
chexel row cy, the fourth byte ignored.  A covered cell is ('▀', fg = RGB8(top), bg = RGB8(bottom)); any other cell is
(' ', RGB8(palette[default_fg]), RGB8(palette[default_bg])) with RGB8 = chexel_restatement.srgb8_v, the encoder's own formula.

The delta keeps `shown`, what the terminal displays, in the same layout: a covered cell is changed when any of its six channels is more
than `tol` away from shown; emitted cells, runs and moves are ansi_delta_restatement's; the new shown is cur where a covered cell was
emitted and shown everywhere else.
"""
from __future__ import annotations

import numpy as np

import ansi_delta_restatement as D
import chexel_restatement as CR

UPPER_HALF = "▀"
INFO = D.INFO


def palette_rgb():
    """RGB8(palette16[k]) for k = 0..15"""
    return [tuple(int(v) for v in CR.srgb8_v(CR._clamp01_v(CR.PALETTE16[k]).astype(np.float64))) for k in range(16)]


def bound(console_w: int, console_h: int) -> int:
    """ESC[2J ESC[H, ESC[0m, each row's ESC[<y+1>;1H, 39 bytes a cell (the longest escape, 7 + 11 + 6 + 11 + 1 = 36, and '▀', 3)"""
    return 7 + 4 + sum(5 + len(str(y + 1)) for y in range(console_h)) + 39 * console_w * console_h


def cells(rgba, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0):
    """the console's cells: covered (ch, cw) bool, fg and bg (ch, cw, 3) int - the defaults where the framebuffer does not reach"""
    rgba = np.asarray(rgba)
    fbH, fbW = rgba.shape[0] // 2, rgba.shape[1]
    assert rgba.shape == (2 * fbH, fbW, 4)
    pal = palette_rgb()
    covered = np.zeros((console_h, console_w), bool)
    fg = np.empty((console_h, console_w, 3), np.int64); fg[...] = pal[default_fg]
    bg = np.empty((console_h, console_w, 3), np.int64); bg[...] = pal[default_bg]
    fx, fy = np.arange(console_w) - viewport[0], np.arange(console_h) - viewport[1]
    in_x, in_y = (fx >= 0) & (fx < fbW), (fy >= 0) & (fy < fbH)
    if in_x.any() and in_y.any():
        at = np.ix_(in_y, in_x)
        covered[at] = True
        fg[at] = rgba[np.ix_(2 * fy[in_y], fx[in_x])][..., :3]
        bg[at] = rgba[np.ix_(2 * fy[in_y] + 1, fx[in_x])][..., :3]
    return covered, fg, bg


def _sgr(fg, bg, cur_fg, cur_bg) -> bytes:
    """the three branches for triples (fg, bg) behind (cur_fg, cur_bg) (None: nothing yet)"""
    if fg != cur_fg and bg != cur_bg:
        return b"\x1b[38;2;%d;%d;%d;48;2;%d;%d;%dm" % (fg + bg)
    if fg != cur_fg:
        return b"\x1b[38;2;%d;%d;%dm" % fg
    if bg != cur_bg:
        return b"\x1b[48;2;%d;%d;%dm" % bg
    return b""


def _triples(a):
    """(ch, cw, 3) -> rows of tuples"""
    return [[tuple(v) for v in row] for row in a.tolist()]


def stream(rgba, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, clear=False) -> bytes:
    covered, fg, bg = cells(rgba, console_w, console_h, viewport, default_fg, default_bg)
    fg, bg, covered = _triples(fg), _triples(bg), covered.tolist()
    out = bytearray(b"\x1b[2J\x1b[H" if clear else b"")
    cur_fg = cur_bg = None
    block = UPPER_HALF.encode("utf-8")
    for y in range(console_h):
        out += b"\x1b[%d;1H" % (y + 1)
        for x in range(console_w):
            out += _sgr(fg[y][x], bg[y][x], cur_fg, cur_bg)
            cur_fg, cur_bg = fg[y][x], bg[y][x]
            out += block if covered[y][x] else b" "
    out += b"\x1b[0m"
    return bytes(out)


def _opaque(rgba):
    out = np.array(rgba, dtype=np.uint8, copy=True)
    out[..., 3] = 255
    return out


def delta(shown, cur, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, gap=3, tol=0, clear=False, keyframe=False):
    """(bytes, info, new shown) of the stream that follows a terminal showing `shown` (an RGBA plane, or None: nothing valid) with `cur`"""
    cur = np.asarray(cur, dtype=np.uint8)
    if shown is None or clear or keyframe:
        return stream(cur, console_w, console_h, viewport, default_fg, default_bg, clear), dict(zip(INFO, (1, 0, 0, 0))), _opaque(cur)
    shown = np.asarray(shown, dtype=np.uint8)
    assert shown.shape == cur.shape and 0 <= gap <= 8 and 0 <= tol <= 255
    covered, fg, bg = cells(cur, console_w, console_h, viewport, default_fg, default_bg)
    _, sfg, sbg = cells(shown, console_w, console_h, viewport, default_fg, default_bg)
    diff = np.maximum(np.abs(fg - sfg).max(axis=-1), np.abs(bg - sbg).max(axis=-1))
    changed = covered & (diff > tol)
    em = D.emitted_mask(changed, gap)
    tfg, tbg = _triples(fg), _triples(bg)
    out = bytearray()
    runs = 0
    new_shown = _opaque(shown)
    block = UPPER_HALF.encode("utf-8")
    for y, x in np.argwhere(em):                               # (raster order)
        y, x = int(y), int(x)
        if x == 0 or not em[y, x - 1]:
            out += b"\x1b[%d;%dH" % (y + 1, x + 1)
            out += _sgr(tfg[y][x], tbg[y][x], None, None)
            runs += 1
        else:
            out += _sgr(tfg[y][x], tbg[y][x], tfg[y][x - 1], tbg[y][x - 1])
        out += block if covered[y, x] else b" "
        if covered[y, x]:
            cx, cy = x - viewport[0], y - viewport[1]
            new_shown[2 * cy, cx, :3] = cur[2 * cy, cx, :3]
            new_shown[2 * cy + 1, cx, :3] = cur[2 * cy + 1, cx, :3]
    out += b"\x1b[0m"
    return bytes(out), dict(zip(INFO, (0, int(changed.sum()), int(em.sum()), runs))), new_shown


def frame_rgba(sdr):
    """the RGBA plane of a frame whose SDR array (fbH, fbW, 2, 3) is given: srgb8_v of its clamped channels"""
    sdr = np.asarray(sdr, dtype=np.float32)
    h, w = sdr.shape[:2]
    s8 = CR.srgb8_v(CR._clamp01_v(sdr).astype(np.float64))                 # (h, w, 2, 3)
    rgba = np.full((h, 2, w, 4), 255, np.uint8)
    rgba[..., :3] = s8.transpose(0, 2, 1, 3)
    return rgba.reshape(2 * h, w, 4)


def frame_stream(sdr, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, clear=False) -> bytes:
    return stream(frame_rgba(sdr), console_w, console_h, viewport, default_fg, default_bg, clear)


def frame_delta(shown, sdr, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, gap=3, tol=0, clear=False, keyframe=False):
    """delta() of a frame given as its SDR array against `shown` (an RGBA plane as delta() returns it, or None)"""
    return delta(shown, frame_rgba(sdr), console_w, console_h, viewport, default_fg, default_bg, gap, tol, clear, keyframe)


class Screen(D.Screen):
    """A terminal that understands exactly the tokens the 24-bit streams contain - ESC[2J, ESC[H, ESC[r;cH, ESC[38;2;R;G;Bm,
    ESC[48;2;R;G;Bm, ESC[38;2;R;G;B;48;2;R;G;Bm, ESC[0m, ' ' and '▀' - and fails on any other byte.  grid[y][x] = (char, fg, bg) with
    fg / bg triples, or None (never written); cursor = (row, col, pending wrap); colours = (fg, bg), (None, None) after ESC[0m."""

    def _triple(self, s: bytes, i: int):
        r, i = self._number(s, i)
        assert s[i:i + 1] == b";", ("a triple without its green", i)
        g, i = self._number(s, i + 1)
        assert s[i:i + 1] == b";", ("a triple without its blue", i)
        b, i = self._number(s, i + 1)
        assert r <= 255 and g <= 255 and b <= 255
        return (r, g, b), i

    def feed(self, s: bytes):
        i = 0
        while i < len(s):
            if s[i] == 0x20:
                self._put(" "); i += 1
            elif s[i:i + 3] == b"\xe2\x96\x80":
                self._put(UPPER_HALF); i += 3
            elif s[i:i + 4] == b"\x1b[2J":
                self.grid = [[(" ", None, None)] * self.w for _ in range(self.h)]; i += 4
            elif s[i:i + 3] == b"\x1b[H":
                self.cursor = (0, 0, False); i += 3
            elif s[i:i + 4] == b"\x1b[0m":
                self.colours = (None, None); i += 4
            elif s[i:i + 7] in (b"\x1b[38;2;", b"\x1b[48;2;"):
                first_is_fg = s[i:i + 7] == b"\x1b[38;2;"
                v, i = self._triple(s, i + 7)
                if first_is_fg and s[i:i + 6] == b";48;2;":
                    b, i = self._triple(s, i + 6)
                    self.colours = (v, b)
                else:
                    self.colours = (v, self.colours[1]) if first_is_fg else (self.colours[0], v)
                assert s[i:i + 1] == b"m", ("SGR without its m", i)
                i += 1
            elif s[i:i + 2] == b"\x1b[":
                r, i = self._number(s, i + 2)
                assert s[i:i + 1] == b";", ("a cursor move without its column", i)
                c, i = self._number(s, i + 1)
                assert s[i:i + 1] == b"H" and 1 <= r <= self.h and 1 <= c <= self.w, ("cursor move", r, c, i)
                self.cursor = (r - 1, c - 1, False); i += 1
            else:
                raise AssertionError(("a byte no stream contains", i, s[max(0, i - 12):i + 12]))
        return self


def within(screen_a: "Screen", screen_b: "Screen", tol: int) -> bool:
    """the two screens agree on cursor, SGR state and every cell's character, and every channel of every cell is within tol"""
    if screen_a.cursor != screen_b.cursor or screen_a.colours != screen_b.colours:
        return False
    for ra, rb in zip(screen_a.grid, screen_b.grid):
        for a, b in zip(ra, rb):
            if (a is None) != (b is None):
                return False
            if a is None:
                continue
            if a[0] != b[0] or max(abs(p - q) for p, q in zip(a[1] + a[2], b[1] + b[2])) > tol:
                return False
    return True
