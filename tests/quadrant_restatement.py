"""The quadrant-glyph frames restated in numpy, from the contract in include/ycge.h (at ycge_render_frame_quadrants) alone: a chexel's
2 x 2 sub-cell colours, the integer fit of a quadrant block glyph and two colours to them, and the console-wide composite the streams walk.

sub_cells() is binary32 operation by operation - the box sum in row-major order from 0, times 1 / count, then ToneMapper.MapPixel
(ToneMapper.cs:204-260) with MathF.Pow / Max / Min through the oracle's orc_pow / orc_max / orc_min - and the same function gives the frame's
ordinary half-cell form (ss x ss boxes), which tests/test_quadrants_cpu.py pins to the oracle's post stage before anything is compared with
the quadrant form.  fit() is plain integers on the bytes of ansi_rgb_restatement's LinearToSrgb8 (chexel_restatement.srgb8_v).  The bytes
of a stream, a delta and the next shown composite are ansi_layers_restatement.stream_of / delta_of over composite() as they stand.
"""
from __future__ import annotations

import numpy as np

import ansi_layers_restatement as LR
import ansi_rgb_restatement as R
import oracle_binding as ob

f32 = np.float32
GLYPHS = (0x2580, 0x2598, 0x259D, 0x2580, 0x2596, 0x258C, 0x259E, 0x259B)          # by mask: bit 0 = TL, bit 1 = TR, bit 2 = BL in the foreground
WEIGHT = {1: 12, 2: 6, 3: 4, 4: 3}


def _binary(name):
    fn = getattr(ob.lib(), name)

    def apply(a, b):
        a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
        out = np.empty(a.shape, f32)
        flat = out.reshape(-1)
        for i, (x, y) in enumerate(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist())):
            flat[i] = fn(x, y)
        return out
    return apply


def _sat01(v):
    """Saturate01 (ToneMapper.cs:240-245): comparisons, a NaN passes"""
    return np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)


def map_pixel(c, effective):
    """MapPixel on (..., 3) binary32 colours with the frame's constants: gamma 2.2, saturation 2.0, vibrance 0"""
    cs_max, cs_min, cs_pow = _binary("orc_max"), _binary("orc_min"), _binary("orc_pow")
    c = np.asarray(c, f32)
    eff = f32(effective)
    with np.errstate(all="ignore"):
        x = (cs_max(f32(0), c) * eff).astype(f32)
        num = (x * ((f32(2.51) * x).astype(f32) + f32(0.03)).astype(f32)).astype(f32)
        den = ((x * ((f32(2.43) * x).astype(f32) + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)
        y = np.where(den > 0, (num / den).astype(f32), f32(0)).astype(f32)
        y = np.where(y < 0, f32(0), y).astype(f32)
        y = np.where(y > 1, f32(1), y).astype(f32)
        inv_g = f32(f32(1) / cs_max(f32(0.1), f32(2.2))[()])
        v = _sat01(cs_pow(_sat01(y), inv_g))
        r, g, b = v[..., 0], v[..., 1], v[..., 2]
        lum = (((f32(0.2126) * r).astype(f32) + (f32(0.7152) * g).astype(f32)).astype(f32) + (f32(0.0722) * b).astype(f32)).astype(f32)
        chroma = (cs_max(r, cs_max(g, b)) - cs_min(r, cs_min(g, b))).astype(f32)
        fsat = (f32(2.0) * (f32(1) + (f32(0.0) * (f32(1) - chroma).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        out = np.stack([_sat01((lum + ((ch - lum).astype(f32) * fsat).astype(f32)).astype(f32)) for ch in (r, g, b)], axis=-1)
    return out.astype(f32)


def _boxes(hdr, fbW, fbH, x_of, y_of, cols, rows):
    """per chexel and box the binary32 sum of cols x rows samples from (x_of, y_of), rows outer, columns inner, from 0, times 1 / (cols rows)"""
    cy, cx = np.mgrid[0:fbH, 0:fbW]
    out = []
    with np.errstate(all="ignore"):
        for x0, y0 in zip(x_of(cx), y_of(cy)):
            s = np.zeros((fbH, fbW, 3), f32)
            for sy in range(rows):
                for sx in range(cols):
                    s = (s + hdr[y0 + sy, x0 + sx]).astype(f32)
            out.append((s * f32(f32(1.0) / f32(cols * rows))).astype(f32))
    return np.stack(out, axis=2)                                           # (fbH, fbW, boxes, 3)


def sub_cells(hdr, fbW, fbH, ss, exposure, quadrants=True):
    """(fbH, fbW, 4, 3) f32 {TL, TR, BL, BR} of the hi-res buffer hdr (fbH*2*ss, fbW*ss, 3) under the effective exposure; ss even.
    quadrants=False: the frame's own (fbH, fbW, 2, 3) {top, bottom} half-cells, ss x ss boxes, any ss"""
    hdr = np.asarray(hdr, f32).reshape(fbH * 2 * ss, fbW * ss, 3)
    if not quadrants:
        avg = _boxes(hdr, fbW, fbH, lambda cx: [cx * ss, cx * ss], lambda cy: [cy * 2 * ss, (cy * 2 + 1) * ss], ss, ss)
    else:
        assert ss >= 2 and ss % 2 == 0, ss
        h = ss // 2
        avg = _boxes(hdr, fbW, fbH, lambda cx: [cx * ss, cx * ss + h, cx * ss, cx * ss + h],
                     lambda cy: [cy * 2 * ss, cy * 2 * ss, (cy * 2 + 1) * ss, (cy * 2 + 1) * ss], h, ss)
    return map_pixel(avg, exposure)


def quadrant_bytes(quad_sdr):
    """Q: (..., 4, 3) int64, the sRGB8 byte of every sub-cell channel as the RGBA plane of the chexel call would hold it"""
    q = np.asarray(quad_sdr, f32).reshape(-1, 4, 3)
    return R.CR.srgb8_v(R.CR._clamp01_v(q).astype(np.float64)).astype(np.int64)


def score(Q, m):
    """score(m) of one cell's bytes Q (4, 3)"""
    F = [k for k in range(3) if m >> k & 1]
    B = [k for k in range(4) if k not in F]
    s = WEIGHT[len(B)] * sum(int(sum(int(Q[k][c]) for k in B)) ** 2 for c in range(3))
    if F:
        s += WEIGHT[len(F)] * sum(int(sum(int(Q[k][c]) for k in F)) ** 2 for c in range(3))
    return s


def fit_cell(Q, min_contrast=0):
    """(m, fg, bg) of one cell's bytes Q (4, 3): the rules of the header in plain integers"""
    Q = [[int(v) for v in row] for row in Q]
    mean0 = [(2 * sum(Q[k][c] for k in range(4)) + 4) // 8 for c in range(3)]
    m = 0
    if max(abs(Q[k][c] - mean0[c]) for k in range(4) for c in range(3)) > min_contrast:
        best = -1
        for cand in range(8):
            s = score(Q, cand)
            if s > best:
                best, m = s, cand
    F = [k for k in range(3) if m >> k & 1]
    B = [k for k in range(4) if k not in F]
    mean = lambda ks: tuple((2 * sum(Q[k][c] for k in ks) + len(ks)) // (2 * len(ks)) for c in range(3))
    bg = mean(B)
    return m, (mean(F) if F else bg), bg


def fit_bytes(Q, min_contrast=0):
    """fit_cell over (n, 4, 3) bytes, vectorised: (masks (n,), fg (n, 3), bg (n, 3)) int64"""
    Q = np.asarray(Q, np.int64).reshape(-1, 4, 3)
    n = Q.shape[0]
    S0 = Q.sum(axis=1)
    mean0 = (2 * S0 + 4) // 8
    flat = np.abs(Q - mean0[:, None, :]).max(axis=(1, 2)) <= min_contrast
    sel = np.array([[m >> k & 1 for k in range(4)] for m in range(8)], np.int64)          # (8, 4): the foreground of every mask
    nf = sel.sum(axis=1)
    SF = np.einsum("mk,nkc->nmc", sel, Q)
    SB = S0[:, None, :] - SF
    wf = np.array([0 if v == 0 else WEIGHT[int(v)] for v in nf], np.int64)
    wb = np.array([WEIGHT[int(4 - v)] for v in nf], np.int64)
    scores = wb[None, :] * (SB * SB).sum(axis=2) + wf[None, :] * (SF * SF).sum(axis=2)
    m = np.where(flat, 0, np.argmax(scores, axis=1))                       # (argmax: the first of the largest)
    idx = np.arange(n)
    sf, sb, f, b = SF[idx, m], SB[idx, m], nf[m][:, None], (4 - nf[m])[:, None]
    bg = (2 * sb + b) // (2 * b)
    fg = np.where(f > 0, (2 * sf + f) // np.maximum(2 * f, 1), bg)
    return m.astype(np.int64), fg, bg


def fit(quad_sdr, min_contrast=0):
    """(glyphs (n,) uint16, fg (n, 3) uint8, bg (n, 3) uint8, masks (n,)) of n cells of sub-cell colours (n, 4, 3) or (n, 12) f32"""
    m, fg, bg = fit_bytes(quadrant_bytes(np.asarray(quad_sdr, f32).reshape(-1, 4, 3)), min_contrast)
    return np.array(GLYPHS, np.uint16)[m], fg.astype(np.uint8), bg.astype(np.uint8), m


def planes(quad_sdr, fbW, fbH, min_contrast=0):
    """the frame's planes: glyphs (fbH, fbW) uint16 and the (2 fbH, fbW, 4) RGBA plane, row 2 cy the foreground, alpha 255"""
    g, fg, bg, _ = fit(quad_sdr, min_contrast)
    rgba = np.full((fbH, 2, fbW, 4), 255, np.uint8)
    rgba[:, 0, :, :3] = fg.reshape(fbH, fbW, 3)
    rgba[:, 1, :, :3] = bg.reshape(fbH, fbW, 3)
    return g.reshape(fbH, fbW), rgba.reshape(2 * fbH, fbW, 4)


def composite(glyphs, rgba, layers, raytrace_at, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0):
    """ansi_layers_restatement.composite in 24-bit colour with the fitted glyphs for '▀' in the raytrace framebuffer: (glyphs (ch, cw),
    colours (2 ch, cw, 4)).  No fitted glyph is ' ', so the framebuffer stays opaque under GetChexelForPoint"""
    glyphs = np.asarray(glyphs, np.uint16)
    r = LR.renderer(True, rgba, layers, raytrace_at, viewport, default_fg, default_bg)
    r.frameBuffers[raytrace_at].chars = LR._chars(glyphs)
    out_g = np.zeros((console_h, console_w), np.uint16)
    out_c = np.full((2 * console_h, console_w, 4), 255, np.uint8)
    for y in range(console_h):
        for x in range(console_w):
            ch, fg, bg = r.GetChexelForPoint(x, y)
            out_g[y, x] = ord(ch)
            out_c[2 * y, x, :3], out_c[2 * y + 1, x, :3] = fg, bg
    return out_g, out_c


def stream(glyphs, rgba, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, clear=False, layers=(), raytrace_at=0) -> bytes:
    return LR.stream_of(True, *composite(glyphs, rgba, list(layers), raytrace_at, console_w, console_h, viewport, default_fg, default_bg), clear)


def delta(shown, glyphs, rgba, console_w, console_h, viewport=(0, 0), default_fg=7, default_bg=0, gap=3, tol=0, clear=False, keyframe=False,
          layers=(), raytrace_at=0):
    """(bytes, info, next shown) after a terminal showing the composite `shown` = (glyphs, colours), or None"""
    cur = composite(glyphs, rgba, list(layers), raytrace_at, console_w, console_h, viewport, default_fg, default_bg)
    return LR.delta_of(True, shown, cur, gap, tol, clear, keyframe)
