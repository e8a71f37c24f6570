"""The delta sixel streams and Video mode's pixel plane restated in Python, from the contract in include/ycge.h (at
ycge_render_frame_sixel_delta and ycge_video_blit_pixels) alone.

encode_delta() writes the delta stream of two register planes rule by rule: the spans, the header with P2 = 1, the bands up to the last
changed one, a line per register present in a band's span.  apply() shares no code with it: a small sixel interpreter for a stream with
P2 = 1 - a zero bit leaves its pixel alone - that paints over a screen, refuses a pixel painted twice, and, told the plane the stream
is meant to show, refuses a pixel painted outside the changed spans and a changed pixel left unpainted.
video_pixels() is the blit's hi-res samples (video_quadrant_restatement.samples) through LinearToSrgb8 (chexel_restatement.srgb8_v) and the
sixel quantiser (sixel_restatement.quantise).
"""
from __future__ import annotations

import re

import numpy as np

import chexel_restatement as CR
import sixel_restatement as X
import video_quadrant_restatement as VQ

ESC = b"\x1b"


def spans(prev, cur):
    """per band (lo, hi) - the smallest column in which any of its rows differs, the largest such column + 1 - or None"""
    d = np.asarray(prev) != np.asarray(cur)
    out = []
    for k in range(0, d.shape[0], 6):
        cols = np.flatnonzero(d[k:k + 6].any(axis=0))
        out.append((int(cols[0]), int(cols[-1]) + 1) if cols.size else None)
    return out


def delta_header(W, H, viewport) -> bytes:
    return ESC + b"[%d;%dH" % (viewport[1] + 1, viewport[0] + 1) + ESC + b"P0;1q" + b'"1;1;%d;%d' % (W, H) + X.register_definitions()


def encode_delta(prev, cur, viewport=(0, 0)):
    """(stream, info) of the delta from the plane prev to the plane cur (both (H, W), values below 216) at viewport (x, y);
    info = (0, changed bands, pixels painted, lines)"""
    prev, cur = np.asarray(prev), np.asarray(cur)
    assert prev.shape == cur.shape and cur.max() < X.REGISTERS and prev.max() < X.REGISTERS
    H, W = cur.shape
    sp = spans(prev, cur)
    changed = [k for k, s in enumerate(sp) if s is not None]
    bands, painted, n_lines = [], 0, 0
    for k in range(changed[-1] + 1 if changed else 0):
        if sp[k] is None:
            bands.append(b"")
            continue
        lo, hi = sp[k]
        band = cur[6 * k:6 * k + 6]
        painted += (hi - lo) * band.shape[0]
        lines = []
        for c in np.unique(band[:, lo:hi]).tolist():
            six = np.zeros(W, np.int64)
            six[lo:hi] = ((band[:, lo:hi] == c) << np.arange(band.shape[0])[:, None]).sum(axis=0)
            last = int(np.flatnonzero(six)[-1])
            line, x = b"#%d" % c, 0
            while x <= last:
                n = 1
                while x + n <= last and six[x + n] == six[x]:
                    n += 1
                ch = bytes([63 + int(six[x])])
                line += b"!%d%s" % (n, ch) if n >= 4 else ch * n
                x += n
            lines.append(line)
        n_lines += len(lines)
        bands.append(b"$".join(lines))
    return delta_header(W, H, viewport) + b"-".join(bands) + ESC + b"\\", (0, len(changed), painted, n_lines)


_HEAD = re.compile(rb"\x1b\[(\d+);(\d+)H\x1bP0;1q\"1;1;(\d+);(\d+)")


def apply(stream: bytes, screen, cur=None):
    """(the screen after the stream, the mask of the pixels it painted).  screen: the (H, W) plane the terminal shows.  cur: the plane the
    stream is meant to show - a pixel painted outside the changed spans or a changed pixel left unpainted is refused"""
    m = _HEAD.match(stream)
    assert m, stream[:40]
    W, H = int(m.group(3)), int(m.group(4))
    plane = np.array(screen, np.uint8)
    assert plane.shape == (H, W), (plane.shape, H, W)
    assert stream[-2:] == ESC + b"\\"
    body = stream[m.end():-2]
    assert ESC not in body
    painted = np.zeros((H, W), bool)
    x = y = 0
    register = None
    at = 0
    while at < len(body):
        ch = body[at:at + 1]
        if ch == b"#":
            t = re.compile(rb"#(\d+)(;2;\d+;\d+;\d+)?").match(body, at)
            register = int(t.group(1))
            at = t.end()
            continue
        if ch == b"$":
            x = 0
        elif ch == b"-":
            x, y = 0, y + 6
        else:
            n = 1
            if ch == b"!":
                t = re.compile(rb"!(\d+)").match(body, at)
                n, at = int(t.group(1)), t.end()
                ch = body[at:at + 1]
            bitmask = ch[0] - 63
            assert 0 <= bitmask < 64 and register is not None and x + n <= W, (at, ch, x, n, W)
            for r in range(6):
                if bitmask & (1 << r):
                    assert y + r < H, (y, r, H)
                    assert not painted[y + r, x:x + n].any(), ("painted twice", x, y + r)
                    painted[y + r, x:x + n] = True
                    plane[y + r, x:x + n] = register
            x += n
        at += 1
    if cur is not None:
        cur = np.asarray(cur)
        differs = np.asarray(screen) != cur
        allowed = np.zeros((H, W), bool)
        for k in range(0, H, 6):
            cols = np.flatnonzero(differs[k:k + 6].any(axis=0))
            if cols.size:
                allowed[k:k + 6, cols.min():cols.max() + 1] = True
        assert not (painted & ~allowed).any(), ("painted outside the changed spans", np.argwhere(painted & ~allowed)[0].tolist())
        assert not (differs & ~painted).any(), ("a changed pixel was left unpainted", np.argwhere(differs & ~painted)[0].tolist())
    return plane, painted


def video_pixels(frame, srcW, srcH, bpp, fbW, fbH, ss, dither=0):
    """(rgba (H, W, 4) uint8, registers (H, W) uint8) of the blit's hi-res samples, H = 2 fbH ss, W = fbW ss"""
    s = VQ.samples(frame, srcW, srcH, bpp, fbW, fbH, ss)
    b = CR.srgb8_v(s.astype(np.float64)).reshape(s.shape)
    rgba = np.concatenate([b, np.full(b.shape[:2] + (1,), 255, np.uint8)], axis=2).astype(np.uint8)
    return rgba, X.quantise(b, dither)
