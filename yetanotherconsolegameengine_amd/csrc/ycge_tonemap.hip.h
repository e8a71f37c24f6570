// ycge_tonemap.hip.h - ToneMapper.MapPixel on the device and the tone state it reads: the one body every kernel that maps a pixel shares
// (k_tonemap_downsample and k_tonemap_quadrants of ycge_post.hip behind a box sum, k_sixel_pixels of ycge_sixel.hip on a sample as it is).
#pragma once
#include "ycge_rt.hip.h"

namespace ycge {

struct ToneState {                          // ToneMapper fields that change (ToneMapper.cs:13,17)
    float ae_exposure;
    float effective;
    uint32_t count;                         // diagnostics: chunks k_exposure_sum added one by one this frame (0 from the serial form)
    uint32_t pad;
    float log_sum;                          // the frame's logSum and cnt (ToneMapper.cs:63-77) as the sum kernels left them: read by the
    uint32_t samples;                       // test hooks only (ycge_test_post_stage / ycge_test_exposure), nothing on the device reads them
};

// ToneMapper.ToneMapAndEncode + ApplySaturation, ToneMapper.cs:204-260
__device__ __forceinline__ float aces_film(float x)
{
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    const float num = x * (a * x + b);
    const float den = x * (c * x + d) + e;
    float y = den > 0.0f ? num / den : 0.0f;
    if (y < 0.0f) y = 0.0f;
    if (y > 1.0f) y = 1.0f;
    return y;
}
__device__ __forceinline__ F3 map_pixel(F3 hdr, float exposure, float gamma, float saturation, float vibrance)
{
    float r = cs_max(0.0f, hdr.x) * exposure;
    float g = cs_max(0.0f, hdr.y) * exposure;
    float b = cs_max(0.0f, hdr.z) * exposure;
    r = aces_film(r); g = aces_film(g); b = aces_film(b);
    const float inv_gamma = 1.0f / cs_max(0.1f, gamma);
    const float sr = m_pow(clamp01(r), inv_gamma);
    const float sg = m_pow(clamp01(g), inv_gamma);
    const float sb = m_pow(clamp01(b), inv_gamma);
    r = clamp01(sr); g = clamp01(sg); b = clamp01(sb);
    const float y = 0.2126f * r + 0.7152f * g + 0.0722f * b;
    const float maxc = cs_max(r, cs_max(g, b));
    const float minc = cs_min(r, cs_min(g, b));
    const float chroma = maxc - minc;
    const float vib = 1.0f + vibrance * (1.0f - chroma);
    const float f = saturation * vib;
    const float rr = y + (r - y) * f, gg = y + (g - y) * f, bb = y + (b - y) * f;
    return f3(clamp01(rr), clamp01(gg), clamp01(bb));
}

} // namespace ycge
