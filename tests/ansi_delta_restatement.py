"""The delta ANSI stream restated in plain Python - what ycge_render_frame_ansi_delta, ycge_video_blit_ansi_delta and ycge_test_ansi_delta
return - and a terminal model that shows what a stream does to a screen.

The reference has no delta presenter: include/ycge.h defines the bytes.  A keyframe is ansi_stream_restatement.stream; a delta writes
the emitted cells in raster order - the changed ones, the unchanged ones in a gap of at most merge_gap cells between two changed cells
of a row, and always the console's last cell - each run behind a cursor move and the two-index escape, every other emitted cell with
the escape of Render()'s three branches against its left neighbour, then ESC[0m.  The cells come from ansi_stream_restatement's lookup.
"""
from __future__ import annotations

import numpy as np

import ansi_stream_restatement as A
import chexel_restatement as CR

INFO = ("keyframe", "changed", "emitted", "runs")


def _renderer(pairs, viewport, default_fg, default_bg):
    pairs = np.asarray(pairs)
    h, w = pairs.shape[:2]
    fb = A.Framebuffer([[A.UPPER_HALF] * w for _ in range(h)], pairs[..., 0], pairs[..., 1], viewport[0], viewport[1])
    return A.Renderer([fb], default_fg, default_bg)


def _sgr(fg, bg, cur_fg, cur_bg) -> bytes:
    """Render()'s three branches (ANSITerminalRenderer.cs:120-143) for (fg, bg) behind (cur_fg, cur_bg)"""
    if fg != cur_fg and bg != cur_bg:
        return b"\x1b[38;5;%d;48;5;%dm" % (fg, bg)
    if fg != cur_fg:
        return b"\x1b[38;5;%dm" % fg
    if bg != cur_bg:
        return b"\x1b[48;5;%dm" % bg
    return b""


def emitted_mask(changed, gap: int):
    """changed (ch, cw) bool -> emitted: changed, the gaps of at most `gap` cells between two changed cells of a row, the last cell"""
    changed = np.asarray(changed, bool)
    em = changed.copy()
    for y in range(changed.shape[0]):
        xs = np.flatnonzero(changed[y])
        for a, b in zip(xs[:-1], xs[1:]):
            if b - a - 1 <= gap:
                em[y, a:b] = True
    em[-1, -1] = True
    return em


def delta(prev, cur, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, gap=1, clear=False, keyframe=False):
    """(bytes, info) of the stream that follows `prev` (pairs (fbH, fbW, 2), or None: no valid prev) with `cur`"""
    cur = np.asarray(cur)
    if prev is None or clear or keyframe:
        return A.stream(cur, console_w, console_h, viewport, default_fg, default_bg, clear), dict(zip(INFO, (1, 0, 0, 0)))
    prev = np.asarray(prev)
    assert prev.shape == cur.shape and 0 <= gap <= 8
    r = _renderer(cur, viewport, default_fg, default_bg)
    fbH, fbW = cur.shape[:2]
    differs = (prev != cur).any(axis=-1)
    fx, fy = np.arange(console_w) - viewport[0], np.arange(console_h) - viewport[1]
    in_x, in_y = (fx >= 0) & (fx < fbW), (fy >= 0) & (fy < fbH)
    changed = np.zeros((console_h, console_w), bool)          # covered cells whose pair differs from prev's in either byte
    changed[np.ix_(in_y, in_x)] = differs[np.ix_(fy[in_y], fx[in_x])]
    em = emitted_mask(changed, gap)
    out = bytearray()
    runs = 0
    for y, x in np.argwhere(em):                               # (raster order)
        y, x = int(y), int(x)
        ch, fg, bg = r.GetChexelForPoint(x, y)
        if x == 0 or not em[y, x - 1]:
            out += b"\x1b[%d;%dH" % (y + 1, x + 1)
            out += _sgr(fg, bg, -1, -1)
            runs += 1
        else:
            _, lfg, lbg = r.GetChexelForPoint(x - 1, y)
            out += _sgr(fg, bg, lfg, lbg)
        out += ch.encode("utf-8")
    out += b"\x1b[0m"
    return bytes(out), dict(zip(INFO, (0, int(changed.sum()), int(em.sum()), runs)))


def frame_delta(prev_sdr, sdr, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, gap=1, clear=False, keyframe=False):
    """delta() of two frames given as SDR arrays (fbH, fbW, 2, 3): their ANSI pairs by chexel_restatement.encode"""
    prev = None if prev_sdr is None else CR.encode(prev_sdr)[1]
    return delta(prev, CR.encode(sdr)[1], console_w, console_h, viewport, default_fg, default_bg, gap, clear, keyframe)


class Screen:
    """A terminal that understands exactly the tokens these streams contain - ESC[2J, ESC[H, ESC[r;cH, the three SGR forms, ESC[0m,
    ' ' and '▀' - and fails on any other byte.  grid[y][x] = (char, fg, bg) or None (never written); cursor = (row, col, pending wrap);
    colours = (fg, bg), None after ESC[0m."""

    def __init__(self, console_w: int, console_h: int):
        self.w, self.h = console_w, console_h
        self.grid = [[None] * console_w for _ in range(console_h)]
        self.cursor = (0, 0, False)
        self.colours = (None, None)

    def state(self):
        return self.grid, self.cursor, self.colours

    def _number(self, s: bytes, i: int):
        j = i
        while j < len(s) and 0x30 <= s[j] <= 0x39:
            j += 1
        assert j > i, ("a number was expected", i, s[max(0, i - 12):i + 12])
        return int(s[i:j]), j

    def _put(self, ch: str):
        row, col, pending = self.cursor
        assert not pending, "a character behind the last column without a cursor move"
        assert self.colours[0] is not None and self.colours[1] is not None, "a character before any colour was set"
        self.grid[row][col] = (ch, self.colours[0], self.colours[1])
        self.cursor = (row, col, True) if col == self.w - 1 else (row, col + 1, False)

    def feed(self, s: bytes):
        i = 0
        while i < len(s):
            if s[i] == 0x20:
                self._put(" "); i += 1
            elif s[i:i + 3] == b"\xe2\x96\x80":
                self._put(A.UPPER_HALF); i += 3
            elif s[i:i + 4] == b"\x1b[2J":
                self.grid = [[(" ", None, None)] * self.w for _ in range(self.h)]; i += 4
            elif s[i:i + 3] == b"\x1b[H":
                self.cursor = (0, 0, False); i += 3
            elif s[i:i + 4] == b"\x1b[0m":
                self.colours = (None, None); i += 4
            elif s[i:i + 7] in (b"\x1b[38;5;", b"\x1b[48;5;"):
                first_is_fg = s[i:i + 7] == b"\x1b[38;5;"
                v, i = self._number(s, i + 7)
                assert v <= 255
                if first_is_fg and s[i:i + 6] == b";48;5;":
                    b, i = self._number(s, i + 6)
                    assert b <= 255
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
