"""The sixel frames restated in Python, from the contract in include/ycge.h (at ycge_render_frame_sixel) alone: a pixel's colour and
register, the stream of a register plane, its bound, and an independent interpreter of such a stream.

pixels() is the frame's MapPixel of every hi-res sample with no box sum (quadrant_restatement.map_pixel, binary32 operation by operation
through the oracle's MathF) and LinearToSrgb8 of the clamped channels (chexel_restatement.srgb8_v); quantise() is the contract's integer
rule.  encode() writes the stream rule by rule.  decode() shares no code with it: a small sixel interpreter - '#' register selection and
definition, '!' repeats, '$', '-', the raster attributes - that paints a W x H plane and asserts that no pixel is painted twice and that
none is left unpainted.
"""
from __future__ import annotations

import re

import numpy as np

import chexel_restatement as CR
import quadrant_restatement as QR

f32 = np.float32
BAYER = np.array([[0, 8, 2, 10], [12, 4, 14, 6], [3, 11, 1, 9], [15, 7, 13, 5]], np.int64)
REGISTERS = 216
ESC = b"\x1b"


def quantise(rgb8, dither=0):
    """registers (H, W) of the sRGB8 bytes (H, W, 3): level = (v + 25) / 51, or with dither (32 v + 102 D[y & 3][x & 3] + 51) / 1632"""
    v = np.asarray(rgb8).astype(np.int64)
    H, W = v.shape[:2]
    if dither:
        y, x = np.mgrid[0:H, 0:W]
        level = (32 * v + 102 * BAYER[y & 3, x & 3][..., None] + 51) // 1632
    else:
        level = (v + 25) // 51
    return (36 * level[..., 0] + 6 * level[..., 1] + level[..., 2]).astype(np.uint8)


def pixels(hdr, fbW, fbH, ss, exposure, dither=0):
    """(rgba (H, W, 4) uint8, registers (H, W) uint8) of the hi-res buffer hdr (2 fbH ss rows of fbW ss samples) under the effective exposure"""
    H, W = 2 * fbH * ss, fbW * ss
    sdr = QR.map_pixel(np.asarray(hdr, f32).reshape(H, W, 3), exposure)
    b = CR.srgb8_v(CR._clamp01_v(sdr).astype(np.float64)).reshape(H, W, 3)
    rgba = np.concatenate([b, np.full((H, W, 1), 255, np.uint8)], axis=2)
    return rgba, quantise(b, dither)


def bound(W, H):
    """ycge_sixel_stream_bound's value (a Python integer of any size); fits(): the call accepts the geometry"""
    return 3200 + -(-H // 6) * min(REGISTERS, 6 * W) * (W + 5)


def fits(W, H):
    return W > 0 and H > 0 and bound(W, H) < 2 ** 32


def register_definitions() -> bytes:
    return b"".join(b"#%d;2;%d;%d;%d" % (i, 20 * (i // 36), 20 * (i // 6 % 6), 20 * (i % 6)) for i in range(REGISTERS))


def encode(index, viewport=(0, 0), clear=False) -> bytes:
    """the stream of a register plane (H, W) at viewport (x, y)"""
    p = np.asarray(index)
    H, W = p.shape
    assert p.max() < REGISTERS
    out = [ESC + b"[2J" if clear else b"", ESC + b"[%d;%dH" % (viewport[1] + 1, viewport[0] + 1), ESC + b"Pq", b'"1;1;%d;%d' % (W, H), register_definitions()]
    bands = []
    for k in range(0, H, 6):
        band = p[k:k + 6]
        lines = []
        for c in np.unique(band).tolist():
            six = ((band == c) << np.arange(band.shape[0])[:, None]).sum(axis=0)
            last = int(np.flatnonzero(six)[-1])
            six = six[:last + 1]
            starts = np.flatnonzero(np.concatenate([[True], six[1:] != six[:-1]]))
            lengths = np.diff(np.concatenate([starts, [last + 1]]))
            line = b"#%d" % c
            for s, n in zip(six[starts].tolist(), lengths.tolist()):
                ch = bytes([63 + s])
                line += b"!%d%s" % (n, ch) if n >= 4 else ch * n
            lines.append(line)
        bands.append(b"$".join(lines))
    out += [b"-".join(bands), ESC + b"\\"]
    return b"".join(out)


def decode(stream: bytes):
    """(registers (H, W) uint8, viewport (x, y), clear, palette {register: (r, g, b) percentages}) of a stream, by interpretation"""
    pos = 0
    clear = stream.startswith(ESC + b"[2J")
    if clear:
        pos = 4
    m = re.compile(rb"\x1b\[(\d+);(\d+)H\x1bPq\"1;1;(\d+);(\d+)").match(stream, pos)
    assert m, stream[:40]
    vy, vx, W, H = (int(g) for g in m.groups())
    pos = m.end()
    assert stream.endswith(ESC + b"\\")
    body = stream[pos:-2]
    assert ESC not in body
    plane = np.full((H, W), 255, np.uint8)
    painted = np.zeros((H, W), bool)
    palette = {}
    x = y = 0
    register = None
    token = re.compile(rb"#(\d+)(?:;(\d+);(\d+);(\d+);(\d+))?|!(\d+)([?-~])|([?-~])|(\$)|(-)")
    at = 0
    while at < len(body):
        t = token.match(body, at)
        assert t, (at, body[at:at + 20])
        at = t.end()
        if t.group(1) is not None:
            register = int(t.group(1))
            if t.group(2) is not None:
                assert t.group(2) == b"2", "RGB colour space"
                palette[register] = (int(t.group(3)), int(t.group(4)), int(t.group(5)))
        elif t.group(8) is not None or t.group(6) is not None:
            n = int(t.group(6)) if t.group(6) is not None else 1
            bits = (t.group(7) or t.group(8))[0] - 63
            assert register is not None and x + n <= W, (x, n, W)
            for r in range(6):
                if bits >> r & 1:
                    assert y + r < H, (y, r, H)
                    assert not painted[y + r, x:x + n].any(), ("painted twice", x, y + r)
                    painted[y + r, x:x + n] = True
                    plane[y + r, x:x + n] = register
            x += n
        elif t.group(9) is not None:
            x = 0
        else:
            x = 0
            y += 6
    assert painted.all(), ("unpainted pixels", int((~painted).sum()))
    return plane, (vx - 1, vy - 1), clear, palette
