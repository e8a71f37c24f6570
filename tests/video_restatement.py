"""A restatement of the reference's Video-mode blit in numpy binary32 (test infrastructure): Renderer/VideoRenderer.cs:68-148 (TryFlipAndBlit)
and :160-291 (Sinc, LanczosKernel, Clamp, SampleSourceLanczos, SampleSourceBilinear, LoadPixel, Clamp01), written from the C# text.  The
reference is C#; no binary of it exists here, so this is the yardstick ycge_video_blit is held to, bit for bit.

Two forms that must agree (tests/test_video_cpu.py):
  blit_scalar   the literal per-sample loop: weights recomputed for every sample, the bilinear fallback included, one np.float32 scalar
                operation per C# operation;
  blit          per-column and per-row tables (the weights depend on the sample column alone / the sample row alone), then the 36
                accumulation steps in the reference's order over whole arrays.
MathF.Sin is the C runtime's sinf: taken from libm through ctypes, as tests/py_restatement.py does.  .NET evaluates float expressions
in binary32, operation by operation (no x87, no contraction): every intermediate below is rounded to np.float32.
"""
import ctypes as C
import ctypes.util

import numpy as np

f32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]

PI = f32(3.14159274)          # MathF.PI
LANCZOS_A = 3                 # :157


def sinf(x) -> np.float32:
    return f32(_libm.sinf(float(x)))


def Sinc(x):                                                   # :160-166
    x = f32(abs(f32(x)))
    if x < f32(1e-6):
        return f32(1.0)
    pix = f32(PI * x)
    return f32(sinf(pix) / pix)


def LanczosKernel(x, a=LANCZOS_A):                             # :169-174
    x = f32(abs(f32(x)))
    if x >= f32(a):
        return f32(0.0)
    return f32(Sinc(x) * Sinc(f32(x / f32(a))))


def Clamp(v, lo, hi):                                          # :177-182
    return lo if v < lo else (hi if v > hi else v)


def Clamp01(v):                                                # :286-291 (= Vec3.Clamp01, Vec3.cs:116-121: -0.0 passes)
    if v < f32(0.0):
        return f32(0.0)
    if v > f32(1.0):
        return f32(1.0)
    return f32(v)


def geometry(srcW, srcH, fbW, fbH, ss):
    """(hiW, hiH, scale, offX, offY) of :36-37 and :75-81"""
    ss = max(1, ss)
    hiW, hiH = fbW * ss, fbH * 2 * ss
    scaleX = f32(f32(hiW) / f32(srcW))
    scaleY = f32(f32(hiH) / f32(srcH))
    scale = scaleX if scaleX < scaleY else scaleY
    dstW = f32(f32(srcW) * scale)
    dstH = f32(f32(srcH) * scale)
    offX = f32(f32(0.5) * f32(f32(hiW) - dstW))
    offY = f32(f32(0.5) * f32(f32(hiH) - dstH))
    return hiW, hiH, scale, offX, offY


def source_position(p, off, scale):                            # :113-116: (x + 0.5f - offX) / scale
    return f32(f32(f32(f32(p) + f32(0.5)) - off) / scale)


def LoadPixel(frame, w, bpp, x, y):                            # :274-283: bytes B G R -> r g b
    o = (y * w + x) * bpp
    bB, bG, bR = int(frame[o]), int(frame[o + 1]), int(frame[o + 2])
    return f32(f32(bR) / f32(255.0)), f32(f32(bG) / f32(255.0)), f32(f32(bB) / f32(255.0))


def SampleSourceBilinear(frame, w, h, bpp, x, y):              # :245-271
    if x < f32(0.0) or y < f32(0.0) or x > f32(w - 1) or y > f32(h - 1):
        return (f32(0.0),) * 3
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    x1 = min(x0 + 1, w - 1)
    y1 = min(y0 + 1, h - 1)
    tx, ty = f32(x - f32(x0)), f32(y - f32(y0))
    c00, c10, c01, c11 = (LoadPixel(frame, w, bpp, a, b) for a, b in ((x0, y0), (x1, y0), (x0, y1), (x1, y1)))
    out = []
    for k in range(3):
        v0 = f32(f32(c00[k] * f32(f32(1.0) - tx)) + f32(c10[k] * tx))
        v1 = f32(f32(c01[k] * f32(f32(1.0) - tx)) + f32(c11[k] * tx))
        out.append(Clamp01(f32(f32(v0 * f32(f32(1.0) - ty)) + f32(v1 * ty))))
    return tuple(out)


def axis_weights(s):
    """one axis of SampleSourceLanczos (:188-221) at source position s: (p0, the six kernel values, their sum)"""
    p0 = int(np.floor(s))
    k, total = [], f32(0.0)
    for ip in range(p0 - (LANCZOS_A - 1), p0 + LANCZOS_A + 1):
        v = LanczosKernel(f32(s - f32(ip)))
        k.append(v)
        total = f32(total + v)
    return p0, k, total


def SampleSourceLanczos(frame, w, h, bpp, x, y):               # :184-241
    if w <= 0 or h <= 0:
        return (f32(0.0),) * 3
    x0, wx, sumWx = axis_weights(x)
    y0, wy, sumWy = axis_weights(y)
    if sumWx <= f32(0.0) or sumWy <= f32(0.0):
        return SampleSourceBilinear(frame, w, h, bpp, x, y)
    invWx, invWy = f32(f32(1.0) / sumWx), f32(f32(1.0) / sumWy)
    wx = [f32(v * invWx) for v in wx]
    wy = [f32(v * invWy) for v in wy]
    rAcc = gAcc = bAcc = f32(0.0)
    for j in range(6):
        sy = Clamp(y0 - 2 + j, 0, h - 1)
        for i in range(6):
            sx = Clamp(x0 - 2 + i, 0, w - 1)
            r, g, b = LoadPixel(frame, w, bpp, sx, sy)
            wxy = f32(wx[i] * wy[j])
            rAcc = f32(rAcc + f32(r * wxy))
            gAcc = f32(gAcc + f32(g * wxy))
            bAcc = f32(bAcc + f32(b * wxy))
    return Clamp01(rAcc), Clamp01(gAcc), Clamp01(bAcc)


def blit_scalar(frame, srcW, srcH, bpp, fbW, fbH, ss) -> np.ndarray:
    """TryFlipAndBlit (:68-131), sample by sample: the SDR array (fbH, fbW, 2, 3) = {topAvg, botAvg} per chexel"""
    frame = np.ascontiguousarray(frame, np.uint8).ravel()
    ss = max(1, ss)
    hiW, hiH, scale, offX, offY = geometry(srcW, srcH, fbW, fbH, ss)
    out = np.zeros((fbH, fbW, 2, 3), f32)
    inv = f32(f32(1.0) / f32(ss * ss))
    for cy in range(fbH):
        for cx in range(fbW):
            for half, yPx0 in ((0, cy * 2 * ss), (1, (cy * 2 + 1) * ss)):
                acc = [f32(0.0)] * 3
                for sy in range(ss):
                    for sx in range(ss):
                        c = SampleSourceLanczos(frame, srcW, srcH, bpp, source_position(cx * ss + sx, offX, scale), source_position(yPx0 + sy, offY, scale))
                        acc = [f32(a + v) for a, v in zip(acc, c)]
                out[cy, cx, half] = [Clamp01(f32(a * inv)) for a in acc]
    return out


def axis_table(n, off, scale):
    """(p0 int32[n], w f32[n, 6], sums f32[n]) of the n hi-res positions of one axis; w is normalised where the sum is > 0"""
    p0, w, sums = np.zeros(n, np.int32), np.zeros((n, 6), f32), np.zeros(n, f32)
    for p in range(n):
        i0, k, total = axis_weights(source_position(p, off, scale))
        p0[p], sums[p] = i0, total
        if total > f32(0.0):
            inv = f32(f32(1.0) / total)
            w[p] = [f32(v * inv) for v in k]
    return p0, w, sums


def tables(srcW, srcH, fbW, fbH, ss):
    """(x0, wx, y0, wy, (scale, offX, offY)): what ycge_host_video_tables returns"""
    hiW, hiH, scale, offX, offY = geometry(srcW, srcH, fbW, fbH, ss)
    x0, wx, sx = axis_table(hiW, offX, scale)
    y0, wy, sy = axis_table(hiH, offY, scale)
    assert (sx > 0).all() and (sy > 0).all(), "a weight sum <= 0: the bilinear fallback is the scalar form's"
    return x0, wx, y0, wy, (scale, offX, offY)


def blit(frame, srcW, srcH, bpp, fbW, fbH, ss) -> np.ndarray:
    """The same SDR array from the two tables: 36 accumulation steps in j, i order over all hi-res samples at once, then the ss x ss sums
    in sy, sx order.  Every array operation is one binary32 operation per element."""
    ss = max(1, ss)
    px = np.ascontiguousarray(frame, np.uint8).reshape(srcH, srcW, bpp)
    unit = (px[..., 2::-1].astype(f32) / f32(255.0)).astype(f32)          # (srcH, srcW, 3) r g b  (:280-282)
    x0, wx, y0, wy, _ = tables(srcW, srcH, fbW, fbH, ss)
    hiW, hiH = fbW * ss, fbH * 2 * ss
    acc = np.zeros((hiH, hiW, 3), f32)
    for j in range(6):
        rows = np.clip(y0 - 2 + j, 0, srcH - 1)
        for i in range(6):
            cols = np.clip(x0 - 2 + i, 0, srcW - 1)
            wxy = (wx[None, :, i] * wy[:, None, j]).astype(f32)          # wx[i] * wyj (:233)
            acc = (acc + (unit[rows[:, None], cols[None, :]] * wxy[..., None]).astype(f32)).astype(f32)
    acc = np.where(acc < f32(0.0), f32(0.0), np.where(acc > f32(1.0), f32(1.0), acc)).astype(f32)      # Clamp01 (:240)
    s = acc.reshape(fbH, 2, ss, fbW, ss, 3)                                  # hi-res row = (2 cy + half) ss + sy, column = cx ss + sx
    total = np.zeros((fbH, 2, fbW, 3), f32)
    for sy in range(ss):
        for sx in range(ss):
            total = (total + s[:, :, sy, :, sx, :]).astype(f32)
    avg = (total * f32(f32(1.0) / f32(ss * ss))).astype(f32)
    avg = np.where(avg < f32(0.0), f32(0.0), np.where(avg > f32(1.0), f32(1.0), avg)).astype(f32)      # Saturate (:127-128)
    return np.ascontiguousarray(avg.transpose(0, 2, 1, 3))
