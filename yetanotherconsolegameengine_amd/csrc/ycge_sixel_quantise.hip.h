// ycge_sixel_quantise.hip.h - a sample's sRGB8 word and its register of the 6 x 6 x 6 cube from its three clamped channels: the one body of
// k_sixel_pixels (ycge_sixel.hip, behind map_pixel) and k_video_pixels (ycge_video.hip, behind the Lanczos sample).  The contract's integer
// rules: include/ycge.h at ycge_render_frame_sixel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_srgb8.hip.h"

namespace ycge_sixel {

// the 4 x 4 Bayer matrix of the dithered quantiser, D[y & 3][x & 3]
static __constant__ uint8_t c_bayer[16] = {0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5};

// a byte's cube level 0..5
template <bool DITHER>
__device__ __forceinline__ uint32_t cube_level(uint32_t v, uint32_t d)
{
    return DITHER ? (32u * v + 102u * d + 51u) / 1632u : (v + 25u) / 51u;
}

// channels in 0..1 (Clamp01'd by the caller) of the hi-res pixel (x, y): the RGBA8 word, alpha 255, and the register.  t32: the 256 thresholds
template <bool DITHER>
__device__ __forceinline__ void word_and_register(float cr, float cg, float cb, const float *t32, uint32_t x, uint32_t y, uint32_t &rgba, uint32_t &reg)
{
    const uint32_t r = (uint32_t)ycge_chexel::srgb8(t32, cr);
    const uint32_t g = (uint32_t)ycge_chexel::srgb8(t32, cg);
    const uint32_t b = (uint32_t)ycge_chexel::srgb8(t32, cb);
    const uint32_t d = DITHER ? (uint32_t)c_bayer[(y & 3u) * 4u + (x & 3u)] : 0u;
    rgba = r | g << 8 | b << 16 | 0xff000000u;
    reg = 36u * cube_level<DITHER>(r, d) + 6u * cube_level<DITHER>(g, d) + cube_level<DITHER>(b, d);
}

} // namespace ycge_sixel
