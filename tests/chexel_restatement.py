"""A numpy restatement of the presenters' colour maps that ycge_render_frame_chexels computes on the device.

Reference (ConsoleGame/Renderer/):
  console-16  Chexel.cs:37-41 (ChexelColor(Vec3) = Clamp01 then NearestConsoleColorFrom), :70-89 (the search), :92-98 (Clamp01),
              palette :11-29.  One byte a chexel: color_16(top) | color_16(bottom) << 4 (Win32's MapAttributes(fg, bg) low byte,
              fg = top, bg = bottom: RayTracing/RaytraceRenderer.cs:260).
  ANSI-256    ANSITerminalRenderer.cs:246-274 (ChexelToAnsi256), :276-284 (ToCubeLevelSrgb), :287-296 (LinearToSrgb8), :317-322
              (Dist2Srgb).  s_graySrgb (:26) is never filled, so the gray candidate is black (:272).
  sRGB8       OpenGLTerminalRenderer.cs:114-145 (the compose image), :390-400 (LinearToSrgb8, the same function).

The scalar functions below follow the reference statement by statement: math.pow (the C library's pow, which Math.Pow calls on Linux),
Python's round (half to even, as Math.Round), binary32 arithmetic through np.float32.  The vectorised ones give the same bytes faster:
numpy's pow may differ from the C library's in the last bit, so every value whose s * 255 lies within 1e-9 of a half-integer is
recomputed with the scalar function (an ulp of pow moves s * 255 by about 1e-13).
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32

# Chexel.cs:11-29
PALETTE16 = np.array([
    [0.00, 0.00, 0.00], [0.00, 0.00, 0.50], [0.00, 0.50, 0.00], [0.00, 0.50, 0.50],
    [0.50, 0.00, 0.00], [0.50, 0.00, 0.50], [0.50, 0.50, 0.00], [0.75, 0.75, 0.75],
    [0.50, 0.50, 0.50], [0.00, 0.00, 1.00], [0.00, 1.00, 0.00], [0.00, 1.00, 1.00],
    [1.00, 0.00, 0.00], [1.00, 0.00, 1.00], [1.00, 1.00, 0.00], [1.00, 1.00, 1.00]], dtype=F32)
CUBE_SRGB = (0, 95, 135, 175, 215, 255)        # ANSITerminalRenderer.cs:23
FLT_MAX = F32(3.4028234663852886e38)


# ------------------------------------------------------------------------------------------------------------ scalar statements
def clamp01(x):
    """Chexel.cs:92-98 on one binary32 channel: compared in double; NaN and -0.0 pass unchanged."""
    x = F32(x)
    return F32(0.0) if float(x) < 0.0 else (F32(1.0) if float(x) > 1.0 else x)


def color16(rgb) -> int:
    """NearestConsoleColorFrom (Chexel.cs:70-89) of Clamp01(rgb): binary32 distances, strict <, ties to the lower index, all-NaN 0."""
    v = [clamp01(c) for c in rgb]
    best, best_d = 0, FLT_MAX
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(16):
            p = PALETTE16[i]
            dr, dg, db = F32(v[0] - p[0]), F32(v[1] - p[1]), F32(v[2] - p[2])
            d = F32(F32(F32(dr * dr) + F32(dg * dg)) + F32(db * db))
            if d < best_d:
                best_d, best = d, i
    return best


def linear_to_srgb8(c: float) -> int:
    """LinearToSrgb8 (ANSITerminalRenderer.cs:287-296 = OpenGLTerminalRenderer.cs:390-400) on a double."""
    c = float(c)
    if c < 0.0:
        c = 0.0
    if c > 1.0:
        c = 1.0
    s = 12.92 * c if c <= 0.0031308 else 1.055 * math.pow(c, 1.0 / 2.4) - 0.055
    if math.isnan(s):
        return 0              # (int)Math.Round(NaN): int.MinValue before .NET 9, 0 from it - clamped to 0 either way
    v = int(round(s * 255.0))
    return 0 if v < 0 else (255 if v > 255 else v)


def _cube_level(v: int) -> int:
    """ToCubeLevelSrgb, ANSITerminalRenderer.cs:276-284"""
    return 0 if v < 48 else 1 if v < 114 else 2 if v < 154 else 3 if v < 194 else 4 if v < 234 else 5


def ansi256(rgb) -> int:
    """ChexelToAnsi256 (ANSITerminalRenderer.cs:246-274) of the ChexelColor(Vec3) of rgb (its color_f32 is Clamp01'd)."""
    r, g, b = (float(clamp01(c)) for c in rgb)
    r, g, b = (0.0 if x < 0.0 else 1.0 if x > 1.0 else x for x in (r, g, b))
    rs, gs, bs = linear_to_srgb8(r), linear_to_srgb8(g), linear_to_srgb8(b)
    ir, ig, ib = _cube_level(rs), _cube_level(gs), _cube_level(bs)
    idx_cube = 16 + 36 * ir + 6 * ig + ib
    y = linear_to_srgb8(0.2126 * r + 0.7152 * g + 0.0722 * b)
    gray_idx = int(round((y - 8.0) / 10.0))
    gray_idx = 0 if gray_idx < 0 else 23 if gray_idx > 23 else gray_idx
    gray_v = 0                                  # s_graySrgb[gray_idx]: the array is never filled (:26, :272)
    chroma = max(abs(rs - gs), max(abs(rs - bs), abs(gs - bs)))
    d_cube = (rs - CUBE_SRGB[ir]) ** 2 + (gs - CUBE_SRGB[ig]) ** 2 + (bs - CUBE_SRGB[ib]) ** 2
    d_gray = (rs - gray_v) ** 2 + (gs - gray_v) ** 2 + (bs - gray_v) ** 2 + 64 if chroma <= 18 else 2 ** 31 - 1
    return 232 + gray_idx if d_gray < d_cube else idx_cube


# ------------------------------------------------------------------------------------------------------------ vectorised
def _clamp01_v(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)


def srgb8_v(c: np.ndarray) -> np.ndarray:
    """linear_to_srgb8 over a float64 array (see the module text for the near-half-integer recheck)."""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        x = np.where(c < 0.0, 0.0, np.where(c > 1.0, 1.0, c))
        s = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)
        v = s * 255.0
        r = np.rint(v)
        near = np.abs(np.abs(v - np.floor(v)) - 0.5) < 1e-9
        out = np.where(np.isnan(r), 0.0, np.clip(r, 0.0, 255.0)).astype(np.uint8)
    for i in np.flatnonzero(near & (x > 0.0031308)):
        out.flat[i] = linear_to_srgb8(float(x.flat[i]))
    return out


def color16_v(rgb: np.ndarray) -> np.ndarray:
    """color16 over [..., 3] binary32 triples."""
    v = _clamp01_v(rgb)
    best = np.zeros(v.shape[:-1], dtype=np.uint8)
    best_d = np.full(v.shape[:-1], FLT_MAX, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(16):
            dr, dg, db = (v[..., k] - PALETTE16[i, k] for k in range(3))
            d = (dr * dr + dg * dg) + db * db
            take = d < best_d
            best_d = np.where(take, d, best_d)
            best = np.where(take, np.uint8(i), best)
    return best


def ansi256_v(rgb: np.ndarray) -> np.ndarray:
    """ansi256 over [..., 3] binary32 triples."""
    v = _clamp01_v(rgb).astype(np.float64)
    s8 = srgb8_v(v).astype(np.int64)
    rs, gs, bs = s8[..., 0], s8[..., 1], s8[..., 2]
    cube = np.array(CUBE_SRGB, dtype=np.int64)
    lv = lambda t: (t >= 48).astype(np.int64) + (t >= 114) + (t >= 154) + (t >= 194) + (t >= 234)
    ir, ig, ib = lv(rs), lv(gs), lv(bs)
    idx_cube = 16 + 36 * ir + 6 * ig + ib
    with np.errstate(invalid="ignore"):
        y = srgb8_v(0.2126 * v[..., 0] + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]).astype(np.float64)
    gray_idx = np.clip(np.rint((y - 8.0) / 10.0), 0, 23).astype(np.int64)
    chroma = np.maximum(np.abs(rs - gs), np.maximum(np.abs(rs - bs), np.abs(gs - bs)))
    d_cube = (rs - cube[ir]) ** 2 + (gs - cube[ig]) ** 2 + (bs - cube[ib]) ** 2
    d_gray = np.where(chroma <= 18, rs * rs + gs * gs + bs * bs + 64, 2 ** 31 - 1)
    return np.where(d_gray < d_cube, 232 + gray_idx, idx_cube).astype(np.uint8)


def encode(sdr: np.ndarray):
    """The three outputs of ycge_render_frame_chexels for an SDR array of shape (fbH, fbW, 2, 3) f32:
    (color16 (fbH, fbW), ansi (fbH, fbW, 2), rgba (2 fbH, fbW, 4))."""
    sdr = np.asarray(sdr, dtype=F32)
    h, w = sdr.shape[:2]
    c = color16_v(sdr)
    c16 = (c[..., 0] | (c[..., 1] << 4)).astype(np.uint8)
    ansi = ansi256_v(sdr)
    s8 = srgb8_v(_clamp01_v(sdr).astype(np.float64))                 # (h, w, 2, 3)
    rgba = np.empty((h, 2, w, 4), dtype=np.uint8)
    rgba[..., :3] = s8.transpose(0, 2, 1, 3)
    rgba[..., 3] = 255
    return c16, ansi, rgba.reshape(2 * h, w, 4)


def thresholds_from_formula():
    """The two tables the library computes (ycge_host_srgb_thresholds), found again here by bisection over the bit patterns with the
    scalar formula: entry k - 1 the smallest binary32 / binary64 whose byte is >= k."""
    t32, t64 = np.zeros(255, F32), np.zeros(255, np.float64)
    for k in range(1, 256):
        lo, hi = 0, 0x3F800000
        while lo < hi:
            mid = (lo + hi) // 2
            if linear_to_srgb8(float(np.uint32(mid).view(F32))) >= k:
                hi = mid
            else:
                lo = mid + 1
        t32[k - 1] = np.uint32(lo).view(F32)
        lo, hi = 0, 0x3FF0000000000000
        while lo < hi:
            mid = (lo + hi) // 2
            if linear_to_srgb8(float(np.uint64(mid).view(np.float64))) >= k:
                hi = mid
            else:
                lo = mid + 1
        t64[k - 1] = np.uint64(lo).view(np.float64)
    return t32, t64
