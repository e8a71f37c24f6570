"""A literal Python restatement of ANSITerminalRenderer.Render() - the stream that ycge_render_frame_ansi builds on the device.

Reference (ConsoleGame/Renderer/ANSITerminalRenderer.cs): Render() :86-153, GetChexelForPoint :67-84, AppendInt :181-202, AppendCharUtf8
:204-, the zeroSeq trailer :19 / :149.  The cells come as a grid of (char, fg, bg) where fg / bg are already the ANSI-256 indices
(ChexelToAnsi256 of the cell's colours: tests/chexel_restatement.py); one framebuffer at a viewport, as RaytraceEntity sets it up.
"""
from __future__ import annotations

import numpy as np

import chexel_restatement as CR

UPPER_HALF = "▀"          # '▀'


class Framebuffer:
    """Width x Height chexels (char, fg, bg) at (ViewportX, ViewportY); chars[y][x], fg / bg numpy arrays (h, w)."""

    def __init__(self, chars, fg, bg, vx=0, vy=0):
        self.chars, self.fg, self.bg = chars, np.asarray(fg), np.asarray(bg)
        self.Height, self.Width = self.fg.shape
        self.ViewportX, self.ViewportY = vx, vy

    def GetChexel(self, x, y):
        return self.chars[y][x], int(self.fg[y, x]), int(self.bg[y, x])


def default_indices():
    """ansi(palette16[k]) for k = 0..15: ChexelColor(ConsoleColor)'s color_f32 is the palette entry (Chexel.cs:11-29)"""
    return [CR.ansi256(CR.PALETTE16[k]) for k in range(16)]


class Renderer:
    def __init__(self, frame_buffers, default_fg: int, default_bg: int):
        self.frameBuffers = list(frame_buffers)
        pal = default_indices()
        self.default_cell = (" ", pal[default_fg], pal[default_bg])
        self.out = bytearray()

    def GetChexelForPoint(self, screenX, screenY):
        for i in range(len(self.frameBuffers) - 1, -1, -1):
            fb = self.frameBuffers[i]
            fbX = screenX - fb.ViewportX
            fbY = screenY - fb.ViewportY
            if 0 <= fbX < fb.Width and 0 <= fbY < fb.Height:
                chexel = fb.GetChexel(fbX, fbY)
                if chexel[0] != " ":
                    return chexel
        return self.default_cell

    def AppendAscii(self, s: str):
        self.out += s.encode("ascii")

    def AppendInt(self, v: int):
        if v == 0:
            self.out += b"0"
            return
        tmp, digits = v, 0
        while tmp > 0:
            tmp //= 10
            digits += 1
        buf = bytearray(digits)
        pos, val = digits - 1, v
        while val > 0:
            buf[pos] = ord("0") + val % 10
            pos -= 1
            val //= 10
        self.out += buf

    def AppendCharUtf8(self, ch: str):
        self.out += ch.encode("utf-8")

    def Render(self, consoleWidth: int, consoleHeight: int, sizeChanged: bool) -> bytes:
        self.out = bytearray()
        if sizeChanged:
            self.AppendAscii("\x1b[2J\x1b[H")
        currentFgIdx = -1
        currentBgIdx = -1
        for y in range(consoleHeight):
            self.AppendAscii("\x1b[")
            self.AppendInt(y + 1)
            self.AppendAscii(";1H")
            for x in range(consoleWidth):
                ch, fgIdx, bgIdx = self.GetChexelForPoint(x, y)
                if fgIdx != currentFgIdx and bgIdx != currentBgIdx:
                    self.AppendAscii("\x1b[38;5;")
                    self.AppendInt(fgIdx)
                    self.AppendAscii(";48;5;")
                    self.AppendInt(bgIdx)
                    self.AppendAscii("m")
                    currentFgIdx = fgIdx
                    currentBgIdx = bgIdx
                elif fgIdx != currentFgIdx:
                    self.AppendAscii("\x1b[38;5;")
                    self.AppendInt(fgIdx)
                    self.AppendAscii("m")
                    currentFgIdx = fgIdx
                elif bgIdx != currentBgIdx:
                    self.AppendAscii("\x1b[48;5;")
                    self.AppendInt(bgIdx)
                    self.AppendAscii("m")
                    currentBgIdx = bgIdx
                self.AppendCharUtf8(ch)
        self.out += bytes([0x1B, ord("["), ord("0"), ord("m")])          # zeroSeq
        return bytes(self.out)


def stream(pairs, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, clear=False) -> bytes:
    """The stream of a console over one framebuffer of ANSI pairs (fbH, fbW, 2) {fg, bg}, every chexel '▀' (as the raytrace blit
    writes them) - what ycge_render_frame_ansi and ycge_test_ansi_stream return."""
    pairs = np.asarray(pairs)
    h, w = pairs.shape[:2]
    fb = Framebuffer([[UPPER_HALF] * w for _ in range(h)], pairs[..., 0], pairs[..., 1], viewport[0], viewport[1])
    return Renderer([fb], default_fg, default_bg).Render(console_w, console_h, clear)


def bound(console_w: int, console_h: int) -> int:
    """ESC[2J ESC[H, ESC[0m, each row's ESC[<y+1>;1H, 23 bytes a cell (the longest escape, 20, and '▀', 3)"""
    return 7 + 4 + sum(5 + len(str(y + 1)) for y in range(console_h)) + 23 * console_w * console_h


def frame_stream(sdr, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, clear=False) -> bytes:
    """the stream of a frame whose SDR array (fbH, fbW, 2, 3) is given: its ANSI pairs by chexel_restatement.encode"""
    _, ansi, _ = CR.encode(sdr)
    return stream(ansi, console_w, console_h, viewport, default_fg, default_bg, clear)
