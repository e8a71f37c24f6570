"""The adaptive sixel palette restated in numpy, from the contract in include/ycge.h (at ycge_render_frame_sixel_palette) alone: the bins, the
eight cut passes over the boxes, the registers' bytes and percentages, the register plane, the stream and its bound.

Nothing here shares code with csrc/ycge_sixel_host.cpp or the kernels: the boxes are found with one boolean mask a box over the 32 768
bins, where the C++ and the kernels sweep the bins with per-box accumulators.  The stream's body follows the cube stream's rules
(sixel_restatement.encode writes the cube's definitions into its streams, so the body is written out here once more); the independent
interpreter is sixel_restatement.decode, which refuses a pixel painted twice or never: shown() runs it and gives back the percentages
the terminal would show for every pixel.
"""
from __future__ import annotations

import numpy as np

import sixel_restatement as X

ESC = X.ESC
BINS = 32768
COORD = np.stack([np.arange(BINS) >> 10, np.arange(BINS) >> 5 & 31, np.arange(BINS) & 31], axis=1)
MAX_PIXELS = 2 ** 24


def bins_of(rgba):
    """the bin of every pixel of an (H, W, >= 3) byte picture, flat"""
    p = np.asarray(rgba).astype(np.int64)
    return ((p[..., 0] >> 3) << 10 | (p[..., 1] >> 3) << 5 | (p[..., 2] >> 3)).ravel()


def build(rgba):
    """(table [32768] the box of every bin, palette [256, 4] RGBA8 of the bytes m - alpha 255, unused entries zero -, pct [256, 3], n)"""
    p = np.asarray(rgba).astype(np.int64)
    assert p.shape[0] * p.shape[1] <= MAX_PIXELS
    b = bins_of(p)
    cnt = np.bincount(b, minlength=BINS)
    sums = np.stack([np.bincount(b, weights=p[..., k].ravel(), minlength=BINS).astype(np.int64) for k in range(3)], axis=1)
    box = np.zeros(BINS, np.int64)
    n = 1
    for _ in range(8):
        n0, rank = n, 0
        for bx in range(n0):
            sel = box == bx
            occ = sel & (cnt > 0)
            lo, hi = COORD[occ].min(axis=0), COORD[occ].max(axis=0)
            extent = hi - lo
            a = int(np.argmax(extent))                      # the first maximum: r, g, b
            if extent[a] < 1:
                continue
            m = np.bincount(COORD[occ, a], weights=cnt[occ], minlength=32).astype(np.int64)
            total, acc, c = int(m.sum()), 0, int(hi[a]) - 1
            for t in range(int(lo[a]), int(hi[a])):
                acc += int(m[t])
                if 2 * acc >= total:
                    c = t
                    break
            up = sel & (COORD[:, a] > c)
            assert cnt[up].sum() > 0 and cnt[sel & ~up].sum() > 0, "both halves hold pixels"
            box[up] = n0 + rank
            rank += 1
        n = n0 + rank
    assert n <= 256
    palette, pct = np.zeros((256, 4), np.uint8), np.zeros((256, 3), np.uint8)
    for i in range(n):
        sel = box == i
        k = int(cnt[sel].sum())
        m = (2 * sums[sel].sum(axis=0) + k) // (2 * k)
        palette[i, :3], palette[i, 3] = m, 255
        pct[i] = (200 * m + 255) // 510
    return box.astype(np.uint8), palette, pct, n


def remap(rgba, table):
    """the register plane (H, W) of a picture through a table"""
    p = np.asarray(rgba)
    return np.asarray(table, np.uint8)[bins_of(p)].reshape(p.shape[0], p.shape[1])


def bound(W, H):
    """ycge_sixel_palette_stream_bound's value (a Python integer of any size)"""
    return 4700 + -(-H // 6) * min(256, 6 * W) * (W + 5)


def fits(W, H):
    return W > 0 and H > 0 and bound(W, H) < 2 ** 32


def definitions(pct, n) -> bytes:
    return b"".join(b"#%d;2;%d;%d;%d" % (i, pct[i][0], pct[i][1], pct[i][2]) for i in range(n))


def encode(index, pct, n, viewport=(0, 0), clear=False) -> bytes:
    """the stream of a register plane (H, W) under the registers' percentages"""
    p = np.asarray(index)
    H, W = p.shape
    assert p.max() < n <= 256
    out = [ESC + b"[2J" if clear else b"", ESC + b"[%d;%dH" % (viewport[1] + 1, viewport[0] + 1), ESC + b"Pq", b'"1;1;%d;%d' % (W, H), definitions(pct, n)]
    bands = []
    for k in range(0, H, 6):
        band = p[k:k + 6].astype(np.int64)
        lines = []
        for c in np.unique(band).tolist():
            six = ((band == c) << np.arange(band.shape[0])[:, None]).sum(axis=0)
            six = six[:int(np.flatnonzero(six)[-1]) + 1]
            starts = np.flatnonzero(np.concatenate([[True], six[1:] != six[:-1]]))
            lengths = np.diff(np.concatenate([starts, [len(six)]]))
            line = b"#%d" % c
            for s, ln in zip(six[starts].tolist(), lengths.tolist()):
                ch = bytes([63 + s])
                line += b"!%d%s" % (ln, ch) if ln >= 4 else ch * ln
            lines.append(line)
        bands.append(b"$".join(lines))
    return b"".join(out + [b"-".join(bands), ESC + b"\\"])


def stream(rgba, viewport=(0, 0), clear=False, held=None):
    """(the stream, index, palette, pct, n, table) of a picture; held = (table, palette, pct, n): mapped through that palette, no build"""
    table, palette, pct, n = build(rgba) if held is None else held
    index = remap(rgba, table)
    return encode(index, pct, n, viewport, clear), index, palette, pct, n, table


def shown(s: bytes):
    """(percentages (H, W, 3) a terminal shows for the stream - by the independent interpreter -, viewport, clear, registers defined)"""
    plane, vp, clear, palette = X.decode(s)
    assert sorted(palette) == list(range(len(palette))), "registers 0 .. n - 1, each defined"
    lut = np.array([palette[i] for i in range(len(palette))], np.int64)
    assert plane.max() < len(lut)
    return lut[plane], vp, clear, len(palette)
