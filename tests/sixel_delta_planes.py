"""(prev, cur) pairs of register planes for the delta sixel tests (tests/test_sixel_delta_cpu.py, tests/test_gpu_sixel_delta.py): what the
delta encoder's seams are - no change, a lone pixel at either edge and in the partial last band, unchanged bands between changed ones, a
span that starts inside the first four columns or later, one that crosses the walk's 64-column trips and the presence tile at 1024, a
register the band holds only outside its span, every pixel changed, many short bands."""
import numpy as np

import sixel_planes as P

WIDTHS = (1, 5, 63, 64, 65, 129, 1025)
HEIGHTS = (1, 6, 7, 13)
KNOWN = np.array([[0, 0, 0, 0, 215], [0, 7, 7, 7, 7], [0, 7, 7, 7, 7], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [43, 43, 43, 43, 0]], np.uint8)


def _other(v):
    """another register for every pixel: none stays what it was"""
    return ((v.astype(np.int64) + 101) % 216).astype(np.uint8)


def pairs(w, h):
    """[(name, prev, cur)] for a w x h picture"""
    noise, runs, sparse = P.drawn(w, h)
    out = [("identical", runs, runs.copy())]

    def one(name, base, edits):
        cur = base.copy()
        for (y, x), v in edits:
            cur[y, x] = v if v != base[y, x] else (v + 1) % 216
        out.append((name, base, cur))

    one("pixel_in_column_0", runs, [((0, 0), 200)])
    one("pixel_in_the_last_column", sparse, [((h // 2, w - 1), 201)])
    one("pixel_in_the_last_band", runs, [((h - 1, w // 2), 17)])
    if h > 6:
        one("first_and_last_band_only", sparse, [((1, w // 3), 5), ((h - 1, w - 1), 6)])
    for lo in (1, 2, 3, 4, 9):
        if lo + 1 < w:
            one("span_from_column_%d" % lo, runs, [((0, lo), 33), ((h - 1, min(w - 1, lo + 2)), 34)])
    if w > 64:
        cur = runs.copy()
        cur[:, 62:66] = _other(runs[:, 62:66])
        out.append(("span_across_63_64", runs, cur))
    if w > 1024:
        cur = noise.copy()
        cur[0, 1020:1025] = _other(noise[0, 1020:1025])
        out.append(("span_across_the_tile_at_1024", noise, cur))
        one("span_of_almost_everything", sparse, [((0, 1), 9), ((h - 1, 1024), 10)])
    if w >= 5:
        # register 77 stands in the band, but only outside the span of columns 2 .. 3: it gets no line
        base = np.full((h, w), 3, np.uint8)
        base[:, 0] = 77
        base[:, w - 1] = 77
        one("a_register_only_outside_the_span", base, [((0, 2), 4), ((h - 1, 3), 5)])
    out.append(("everything_changed", noise if w <= 129 else runs, _other(noise if w <= 129 else runs)))
    return out


def bands_300():
    prev = P.SEAMS["300_bands_of_8_columns"]()
    cur = prev.copy()
    rows = np.r_[0:6, 600:606, 1794:1800]
    cur[rows, 2:7] = _other(prev[rows, 2:7])
    return [("300_bands_three_changed", prev, cur), ("300_bands_all_changed", prev, _other(prev))]


def adversarial(w, h):
    """planes that make the longest delta streams of a w x h picture: every pixel changed into the plane with the most lines and no runs,
    and the same with only the last band changed (the most '-' in front of the most lines)"""
    idx = np.arange(w * h).reshape(h, w)
    busy = ((idx * 7 + idx // w * 3) % 216).astype(np.uint8)
    prev = _other(busy)
    start = 6 * ((h - 1) // 6)
    tail = busy.copy()
    tail[start:] = prev[start:]
    return [(prev, busy), (tail, busy), (busy, prev)]
