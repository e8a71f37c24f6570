// ycge_video_sample.hip.h - one hi-res sample of Video mode's Lanczos-3 blit: SampleSourceLanczos (Renderer/VideoRenderer.cs:184-241) and its
// Clamp01, operation for operation - the one body of k_video_blit, k_video_blit_quadrants and k_video_pixels (ycge_video.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ycge_video {

// byte / 255.0f, correctly rounded, without the division's expansion: q = b * fl(1/255) is within an ulp, one Newton step on the exact
// residual lands on the quotient (Markstein); equal to the division for all 256 bytes (tests/test_video_cpu.py checks the formula)
__device__ __forceinline__ float unorm8(uint32_t b)
{
    const float k = 1.0f / 255.0f;
    const float x = (float)b;
    const float q = x * k;
    const float r = __builtin_fmaf(-255.0f, q, x);
    return __builtin_fmaf(r, k, q);
}

// VideoRenderer.Clamp01 (:286-291) = Vec3.Clamp01: -0.0 passes
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

__device__ __forceinline__ uint32_t load_pixel(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// The row part of a sample, uniform over the wavefront that shares the hi-res row y: its six weights and the byte offsets of its six tap rows
// (clamped to the frame)
__device__ __forceinline__ void sample_rows(const int32_t *__restrict__ ty0, const float *__restrict__ twy, uint32_t y, int src_h, uint32_t pitch, float wy[6],
                                            uint32_t row[6])
{
    const int y0 = ty0[y];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        wy[j] = twy[(size_t)y * 6 + j];
        const int iy = y0 - 2 + j;
        row[j] = (uint32_t)(iy < 0 ? 0 : (iy > src_h - 1 ? src_h - 1 : iy)) * pitch;
    }
}

// The sample of hi-res column x in the row sample_rows prepared: 36 taps in j (rows), i (columns) order, wxy = wx[i] * wy[j], acc += c * wxy
// per channel, c = byte / 255.0f, tap columns clamped to the frame, Clamp01 per channel
__device__ __forceinline__ void sample(const uint8_t *__restrict__ frame, int src_w, int bpp, const int32_t *__restrict__ tx0, const float *__restrict__ twx, uint32_t x,
                                       const float wy[6], const uint32_t row[6], float &r_out, float &g_out, float &b_out)
{
    const int x0 = tx0[x];
    float wx[6];
    uint32_t col[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        wx[i] = twx[(size_t)x * 6 + i];
        const int ix = x0 - 2 + i;
        col[i] = (uint32_t)(ix < 0 ? 0 : (ix > src_w - 1 ? src_w - 1 : ix)) * (uint32_t)bpp;
    }
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; j++) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const uint32_t px = load_pixel(frame + row[j] + col[i]);          // B G R [A]
            const float wxy = wx[i] * wy[j];
            r += unorm8(px >> 16 & 255u) * wxy;
            g += unorm8(px >> 8 & 255u) * wxy;
            b += unorm8(px & 255u) * wxy;
        }
    }
    r_out = clamp01(r); g_out = clamp01(g); b_out = clamp01(b);
}

} // namespace ycge_video
