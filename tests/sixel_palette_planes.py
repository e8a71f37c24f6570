"""The RGBA planes both adaptive-palette test files use (tests/test_sixel_palette_cpu.py, tests/test_gpu_sixel_palette.py): the smallest
shapes at which the rule or a kernel can go wrong.  PLANES: name -> a function giving (H, W, 4) uint8, alpha 255; HOLD: (first, second)
pairs for the kept palette; expected(): the restatement's answer of a plane, computed once a session and shared read-only."""
from __future__ import annotations

import functools

import numpy as np

import sixel_palette_restatement as R

CANARY = 0xA5


def _rgba(rgb):
    rgb = np.asarray(rgb, np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2))


def flat(w, h, colour):
    return _rgba(np.broadcast_to(np.array(colour, np.uint8), (h, w, 3)))


def two_colour():
    """the contract's known answer: 6 x 12, rows 0..5 black, rows 6..11 white"""
    p = np.zeros((12, 6, 3), np.uint8)
    p[6:] = 255
    return _rgba(p)


def drawn(w, h, seed, spread=256):
    """drawn bytes: a smooth gradient under noise, so that bins are shared and counts differ"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)], axis=-1)
    return _rgba(np.clip(base + rng.integers(-spread // 8, spread // 8 + 1, base.shape), 0, 255))


def every_bin():
    """256 x 128: every bin once (bytes 8 t + 3) - every pass splits every box"""
    t = np.arange(32) * 8 + 3
    r, g, b = np.meshgrid(t, t, t, indexing="ij")
    return _rgba(np.stack([r, g, b], axis=-1).reshape(128, 256, 3))


def clamp_decides():
    """one box whose marginal on r is {1, 0, .., 0, 100}: the median falls on omax, the cut is omax - 1"""
    p = np.zeros((1, 101, 3), np.uint8)
    p[0, 0] = (8, 40, 40)
    p[0, 1:] = (200, 40, 40)
    return _rgba(p)


def ties_two():
    """equal extents on g and b (r flat): g is cut first"""
    p = np.zeros((2, 2, 3), np.uint8)
    p[0, 0], p[0, 1], p[1, 0], p[1, 1] = (80, 16, 16), (80, 16, 120), (80, 120, 16), (80, 120, 120)
    return _rgba(p)


def ties_three():
    """equal extents on all three axes: r is cut first"""
    c = np.array([[8 + 96 * (i >> 2 & 1), 8 + 96 * (i >> 1 & 1), 8 + 96 * (i & 1)] for i in range(8)], np.uint8)
    return _rgba(np.repeat(c.reshape(2, 4, 3), 3, axis=1)[:, :11])


def four_colours():
    """1030 x 7: past the presence tile, W no multiple of 4, H no multiple of 6"""
    y, x = np.mgrid[0:7, 0:1030]
    c = np.array([(10, 10, 10), (250, 20, 30), (30, 240, 20), (20, 30, 245)], np.uint8)
    return _rgba(c[((x // 37) + (y // 2) + (x == 1029)) % 4])


def contended():
    """512 x 512 of one colour but for 3 pixels: the contended bin"""
    p = np.full((512, 512, 3), (97, 160, 229), np.uint8)
    p[0, 0], p[255, 300], p[511, 511] = (0, 0, 0), (255, 255, 255), (96, 161, 228)
    return _rgba(p)


PLANES = {
    "1x1": lambda: flat(1, 1, (1, 2, 3)),
    "5x7_flat": lambda: flat(5, 7, (77, 77, 77)),
    "6x12_two": two_colour,
    "13x11_drawn": lambda: drawn(13, 11, 5),
    "256x128_every_bin": every_bin,
    "clamp": clamp_decides,
    "ties_two": ties_two,
    "ties_three": ties_three,
    "1030x7_four": four_colours,
    "512x512_contended": contended,
    "300x50_drawn": lambda: drawn(300, 50, 9),
}
# what the restatement must say of them (the issue's "checked here" figures among them)
COUNTS = {"1x1": 1, "5x7_flat": 1, "6x12_two": 2, "256x128_every_bin": 256, "clamp": 2, "ties_two": 4, "ties_three": 8, "1030x7_four": 4}
VIEWPORTS = [(0, 0), (2, 1), (9, 99)]


def hold_pair():
    """build on the first; the second has pixels in bins the first left empty"""
    first = drawn(40, 19, 21, spread=64)
    second = drawn(40, 19, 22)
    second[3, 5, :3], second[18, 39, :3] = (255, 0, 255), (0, 255, 0)
    return first, second


@functools.lru_cache(maxsize=None)
def plane(name):
    p = PLANES[name]()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def expected(name, k=0):
    """(stream, index, palette, pct, n, table) of PLANES[name] at VIEWPORTS[k % 3], clear for odd k - the restatement's, made once"""
    out = R.stream(plane(name), VIEWPORTS[k % len(VIEWPORTS)], bool(k & 1))
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
