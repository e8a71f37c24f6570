"""The quadrant form of the Video-mode blit restated in numpy binary32 (test infrastructure), from the contract in include/ycge.h at
ycge_video_blit_quadrants and the samples of tests/video_restatement.py: the yardstick k_video_blit_quadrants is held to, bit for bit.

A sample is SampleSourceLanczos' value after its per-channel Clamp01.  Quadrant k (0 = TL, 1 = TR, 2 = BL, 3 = BR) of chexel (cx, cy) covers
hi-res columns cx ss + (k & 1) ss / 2 .. + ss / 2 - 1 and rows (2 cy + (k >> 1)) ss .. + ss - 1; its colour is the binary32 sum of its
samples, rows outer, columns inner, per channel, from 0, times 1.0f / (float)((ss / 2) ss), through Clamp01.  The SDR beside it is
video_restatement.blit's: the serial sy, sx sum over all ss columns, which the two halves' sums do not add up to in binary32.

Two forms that must agree (tests/test_video_quadrants_cpu.py):
  blit_quadrants_scalar   sample by sample from video_restatement.SampleSourceLanczos, one np.float32 scalar operation per operation;
  blit_quadrants          from video_restatement.tables(), the 36 accumulation steps over all hi-res samples at once, as blit is.
Both return (sdr (fbH, fbW, 2, 3), quad_sdr (fbH, fbW, 4, 3)).  The planes of those sub-cell colours come from quadrant_restatement.planes,
the streams from quadrant_restatement.stream / .delta, unchanged.
"""
import numpy as np

import video_restatement as VR

f32 = np.float32


def _clamp01_v(a):
    return np.where(a < f32(0.0), f32(0.0), np.where(a > f32(1.0), f32(1.0), a)).astype(f32)


def samples(frame, srcW, srcH, bpp, fbW, fbH, ss) -> np.ndarray:
    """(hiH, hiW, 3) f32: every hi-res sample after Clamp01 - video_restatement.blit's accumulation, step for step"""
    px = np.ascontiguousarray(frame, np.uint8).reshape(srcH, srcW, bpp)
    unit = (px[..., 2::-1].astype(f32) / f32(255.0)).astype(f32)
    x0, wx, y0, wy, _ = VR.tables(srcW, srcH, fbW, fbH, ss)
    hiW, hiH = fbW * ss, fbH * 2 * ss
    acc = np.zeros((hiH, hiW, 3), f32)
    for j in range(6):
        rows = np.clip(y0 - 2 + j, 0, srcH - 1)
        for i in range(6):
            cols = np.clip(x0 - 2 + i, 0, srcW - 1)
            wxy = (wx[None, :, i] * wy[:, None, j]).astype(f32)
            acc = (acc + (unit[rows[:, None], cols[None, :]] * wxy[..., None]).astype(f32)).astype(f32)
    return _clamp01_v(acc)


def sums(s, fbW, fbH, ss):
    """the unscaled binary32 sums of the samples s (hiH, hiW, 3): (serial (fbH, 2, fbW, 3) in sy, sx order, halves (fbH, 2, fbW, 2, 3) - per
    half-cell row the left and the right half of the columns, each rows outer, columns inner)"""
    h = ss // 2
    s = s.reshape(fbH, 2, ss, fbW, ss, 3)                                     # hi-res row = (2 cy + half) ss + sy, column = cx ss + sx
    serial = np.zeros((fbH, 2, fbW, 3), f32)
    halves = np.zeros((fbH, 2, fbW, 2, 3), f32)
    for sy in range(ss):
        for sx in range(ss):
            serial = (serial + s[:, :, sy, :, sx, :]).astype(f32)
            halves[:, :, :, sx // h, :] = (halves[:, :, :, sx // h, :] + s[:, :, sy, :, sx, :]).astype(f32)
    return serial, halves


def blit_quadrants(frame, srcW, srcH, bpp, fbW, fbH, ss):
    assert ss >= 2 and ss % 2 == 0, ss
    serial, halves = sums(samples(frame, srcW, srcH, bpp, fbW, fbH, ss), fbW, fbH, ss)
    sdr = _clamp01_v((serial * f32(f32(1.0) / f32(ss * ss))).astype(f32))
    quad = _clamp01_v((halves * f32(f32(1.0) / f32((ss // 2) * ss))).astype(f32))
    # (fbH, half, fbW, side, 3) -> (fbH, fbW, 2 half + side, 3)
    return np.ascontiguousarray(sdr.transpose(0, 2, 1, 3)), np.ascontiguousarray(quad.transpose(0, 2, 1, 3, 4).reshape(fbH, fbW, 4, 3))


def blit_quadrants_scalar(frame, srcW, srcH, bpp, fbW, fbH, ss):
    assert ss >= 2 and ss % 2 == 0, ss
    frame = np.ascontiguousarray(frame, np.uint8).ravel()
    hiW, hiH, scale, offX, offY = VR.geometry(srcW, srcH, fbW, fbH, ss)
    h = ss // 2
    sdr, quad = np.zeros((fbH, fbW, 2, 3), f32), np.zeros((fbH, fbW, 4, 3), f32)
    inv, inv_q = f32(f32(1.0) / f32(ss * ss)), f32(f32(1.0) / f32(h * ss))
    for cy in range(fbH):
        for cx in range(fbW):
            for half in range(2):
                acc = [f32(0.0)] * 3
                q = [[f32(0.0)] * 3, [f32(0.0)] * 3]
                for sy in range(ss):
                    y = VR.source_position((cy * 2 + half) * ss + sy, offY, scale)
                    for sx in range(ss):
                        c = VR.SampleSourceLanczos(frame, srcW, srcH, bpp, VR.source_position(cx * ss + sx, offX, scale), y)
                        acc = [f32(a + v) for a, v in zip(acc, c)]
                        q[sx // h] = [f32(a + v) for a, v in zip(q[sx // h], c)]
                sdr[cy, cx, half] = [VR.Clamp01(f32(a * inv)) for a in acc]
                for side in range(2):
                    quad[cy, cx, 2 * half + side] = [VR.Clamp01(f32(a * inv_q)) for a in q[side]]
    return sdr, quad
