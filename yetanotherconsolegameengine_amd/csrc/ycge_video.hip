// ycge_video.hip - Video mode on the device: VideoRenderer.TryFlipAndBlit's Lanczos-3 blit of a source frame to chexels (host side:
// ycge_video.cpp).
//
// One launch turns the uploaded BGR / BGRA frame into the SDR array {top rgb, bottom rgb} that k_encode_chexels and the ANSI stream
// kernels consume, as Renderer/VideoRenderer.cs:93-131 and SampleSourceLanczos (:184-241) compute it, operation for operation:
//   per hi-res sample  36 taps in j (rows), i (columns) order, wxy = wx[i] * wy[j], acc += c * wxy per channel, c = byte / 255.0f,
//                      tap coordinates clamped to the frame, Clamp01 per channel;
//   per half-cell      the ss * ss samples added in sy, sx order from zero, times 1.0f / (ss * ss), Saturate.
// The weights are separable and come from the host (two small tables made with libm's sinf, the function MathF.Sin calls): per
// hi-res column its x0 = (int)floor(sx) and six normalised weights, per hi-res row the same.  No weight sum is <= 0 (the host checks
// every one), so the reference's bilinear fallback (:215) is never taken and has no branch here.
//
// Mapping: a workgroup is one wavefront on 64 neighbouring chexels of ONE half-cell row, so the row's y0 and weights are uniform
// (scalar loads) and the lanes' taps of one (j, i) lie side by side in the source row.  A tap is one unaligned 32-bit load of its
// pixel - 3-byte pixels included; the last pixel's load reads one byte past the frame, into the padding every DevBuf has.  Neighbouring
// samples share five of six tap columns: those hits are the vector cache's.  A source window staged in LDS was weighed and left out:
// its size is (chexels of the run) / scale + 6 columns by 6 / scale + 6 rows, unbounded when a large frame goes to a small console.
// Its own translation unit, as ycge_chexel.hip is: the code objects of the frame kernels stay what they were.
//
// The quadrant form (k_video_blit_quadrants; the contract: include/ycge.h at ycge_video_blit_quadrants) is the same body with the same
// mapping: beside the SDR it writes each chexel's 2 x 2 sub-cell colours, the sums of the left and right half of a half-cell row's columns,
// for k_fit_quadrants (ycge_chexel.hip).  Per lane 3 floats of the SDR and 6 consecutive floats of quad_sdr; no LDS, no atomics, no scratch.
//
// The pixel plane (k_video_pixels; the contract: include/ycge.h at ycge_video_blit_pixels) is every hi-res sample as it is - its sRGB8 word and
// its register of the sixel cube - for the sixel presenter's encoder (ycge_sixel.hip).  The 36-tap sample is ycge_video_sample.hip.h's, the one
// body of all three kernels.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "ycge_sixel_quantise.hip.h"
#include "ycge_video_sample.hip.h"

namespace {

constexpr int kVideoBlock = 64;

using ycge_video::clamp01;          // unorm8, Clamp01, the pixel load and the 36-tap sample: ycge_video_sample.hip.h

// The blit's body, once for both forms.  Quad: the quadrant form (k_video_blit_quadrants) - beside the serial top / bottom sum, which stays
// what it is sample for sample, the lane keeps the sums of the left and the right half of its columns: quadrants 2 (hy & 1) and 2 (hy & 1) + 1
// of its chexel, rows outer, columns inner, from zero.  The halves are two loops (unrolled: h is a constant in each), so no accumulator is
// indexed by a run-time value; ss is even there (the launcher checks).  The SDR is not made from the quadrant sums: in binary32 the two
// halves do not add up to the serial sum.
// tables: int32 x0[hiW], f32 wx[hiW][6], int32 y0[hiH], f32 wy[hiH][6]
template <bool Quad>
__device__ __forceinline__ void video_blit(const uint8_t *__restrict__ frame, int src_w, int src_h, int bpp, uint32_t fbW, int ss, uint32_t groups_x,
                                           const int32_t *__restrict__ tx0, const float *__restrict__ twx, const int32_t *__restrict__ ty0,
                                           const float *__restrict__ twy, float inv, float *__restrict__ sdr, float inv_quad, float *__restrict__ quad_sdr)
{
    const uint32_t hy = blockIdx.x / groups_x;                   // the half-cell row: 2 cy (top) or 2 cy + 1 (bottom); yTopPx0 / yBotPx0 = hy * ss (:95-96)
    const uint32_t cx = (blockIdx.x - hy * groups_x) * kVideoBlock + threadIdx.x;
    if (cx >= fbW) return;
    const uint32_t pitch = (uint32_t)src_w * (uint32_t)bpp;
    constexpr int kHalves = Quad ? 2 : 1;
    const int span = Quad ? ss >> 1 : ss;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    float q[kHalves][3] = {};
    for (int sy = 0; sy < ss; sy++) {
        const uint32_t y = hy * (uint32_t)ss + (uint32_t)sy;
        float wy[6];
        uint32_t row[6];
        ycge_video::sample_rows(ty0, twy, y, src_h, pitch, wy, row);
#pragma unroll
        for (int h = 0; h < kHalves; h++) {
            for (int sx = h * span; sx < (h + 1) * span; sx++) {
                const uint32_t x = cx * (uint32_t)ss + (uint32_t)sx;
                float r, g, b;
                ycge_video::sample(frame, src_w, bpp, tx0, twx, x, wy, row, r, g, b);
                sum[0] = sum[0] + r;
                sum[1] = sum[1] + g;
                sum[2] = sum[2] + b;
                if constexpr (Quad) {
                    q[h][0] = q[h][0] + r;
                    q[h][1] = q[h][1] + g;
                    q[h][2] = q[h][2] + b;
                }
            }
        }
    }
    float *o = sdr + ((size_t)(hy >> 1) * fbW + cx) * 6 + (hy & 1u) * 3;
    o[0] = clamp01(sum[0] * inv);
    o[1] = clamp01(sum[1] * inv);
    o[2] = clamp01(sum[2] * inv);
    if constexpr (Quad) {
        // {TL rgb, TR rgb, BL rgb, BR rgb} a chexel: this half-cell row's two quadrants are six consecutive floats
        float *p = quad_sdr + ((size_t)(hy >> 1) * fbW + cx) * 12 + (hy & 1u) * 6;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            p[3 * h + 0] = clamp01(q[h][0] * inv_quad);
            p[3 * h + 1] = clamp01(q[h][1] * inv_quad);
            p[3 * h + 2] = clamp01(q[h][2] * inv_quad);
        }
    }
}

__global__ __launch_bounds__(kVideoBlock) void k_video_blit(const uint8_t *__restrict__ frame, int src_w, int src_h, int bpp, uint32_t fbW, int ss, uint32_t groups_x,
                                                            const int32_t *__restrict__ tx0, const float *__restrict__ twx, const int32_t *__restrict__ ty0,
                                                            const float *__restrict__ twy, float inv, float *__restrict__ sdr)
{
    video_blit<false>(frame, src_w, src_h, bpp, fbW, ss, groups_x, tx0, twx, ty0, twy, inv, sdr, 0.0f, nullptr);
}

// the quadrant form: the same samples; sdr as k_video_blit writes it, and quad_sdr, fbW * fbH * 12 floats
__global__ __launch_bounds__(kVideoBlock) void k_video_blit_quadrants(const uint8_t *__restrict__ frame, int src_w, int src_h, int bpp, uint32_t fbW, int ss,
                                                                      uint32_t groups_x, const int32_t *__restrict__ tx0, const float *__restrict__ twx,
                                                                      const int32_t *__restrict__ ty0, const float *__restrict__ twy, float inv,
                                                                      float *__restrict__ sdr, float inv_quad, float *__restrict__ quad_sdr)
{
    video_blit<true>(frame, src_w, src_h, bpp, fbW, ss, groups_x, tx0, twx, ty0, twy, inv, sdr, inv_quad, quad_sdr);
}

// Video mode's pixel plane (the contract: include/ycge.h at ycge_video_blit_pixels): every hi-res sample of the blit as it is - no box sum -
// its sRGB8 word and its register of the sixel cube.  One lane a sample; a wavefront takes 64 neighbouring samples of ONE hi-res row, so the
// row's y0 and six weights are scalar loads (the wavefront's number is made uniform for the compiler) and the lanes' taps of one (j, i) lie
// side by side in the source, as in k_video_blit; a workgroup is four such wavefronts, which share the 256 thresholds in LDS as
// k_sixel_pixels' lanes do.  A wavefront stores 64 consecutive words and 64 consecutive bytes.  Four samples a lane (uint4 and word stores)
// would put four columns' 24 weights and offsets in a lane for stores that are full lines already: the one-sample form is kept.
constexpr int kPixelsBlock = 256;

template <bool DITHER>
__global__ __launch_bounds__(kPixelsBlock) void k_video_pixels(const uint8_t *__restrict__ frame, int src_w, int src_h, int bpp, uint32_t hiW, uint32_t chunks_x,
                                                               uint32_t chunks, const int32_t *__restrict__ tx0, const float *__restrict__ twx,
                                                               const int32_t *__restrict__ ty0, const float *__restrict__ twy, const uint8_t *__restrict__ tables,
                                                               uint32_t *__restrict__ rgba_out, uint8_t *__restrict__ index_out)
{
    __shared__ float t32[256];
    t32[threadIdx.x] = reinterpret_cast<const float *>(tables)[threadIdx.x];
    __syncthreads();
    const uint32_t chunk = blockIdx.x * (kPixelsBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (chunk >= chunks) return;
    const uint32_t y = chunk / chunks_x;
    const uint32_t x = (chunk - y * chunks_x) * 64u + (threadIdx.x & 63u);
    if (x >= hiW) return;
    float wy[6];
    uint32_t row[6];
    ycge_video::sample_rows(ty0, twy, y, src_h, (uint32_t)src_w * (uint32_t)bpp, wy, row);
    float r, g, b;
    ycge_video::sample(frame, src_w, bpp, tx0, twx, x, wy, row, r, g, b);
    uint32_t word, reg;
    ycge_sixel::word_and_register<DITHER>(r, g, b, t32, x, y, word, reg);
    const size_t at = (size_t)y * hiW + x;
    if (rgba_out) rgba_out[at] = word;
    if (index_out) index_out[at] = (uint8_t)reg;
}

} // namespace

namespace {

// what both launchers refuse, and the grid: one wavefront for 64 chexels of one half-cell row
bool video_launch_shape(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, const float *sdr, uint32_t &groups_x,
                        uint32_t &groups)
{
    if (!frame || !tables || !sdr || src_w < 1 || src_h < 1 || (bpp != 3 && bpp != 4) || (int64_t)src_w * src_h * bpp > (int64_t)INT32_MAX || fbW < 1 || fbH < 1 ||
        ss < 1 || ss > 4096 || (int64_t)fbW * ss > (int64_t)INT32_MAX / 8 || (int64_t)fbH * 2 * ss > (int64_t)INT32_MAX / 8 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return false;
    groups_x = ((uint32_t)fbW + kVideoBlock - 1) / kVideoBlock;
    const uint64_t n = (uint64_t)groups_x * 2u * (uint32_t)fbH;
    if (n > (uint64_t)INT32_MAX) return false;
    groups = (uint32_t)n;
    return true;
}

} // namespace

// frame: src_w * src_h * bpp bytes in an allocation with at least one byte of padding behind them; tables as above for hiW = fbW * ss
// columns and hiH = fbH * 2 * ss rows; sdr: fbW * fbH * 6 floats
extern "C" int ycge_launch_video_blit(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, float *sdr,
                                      hipStream_t stream)
{
    uint32_t groups_x = 0, groups = 0;
    if (!video_launch_shape(frame, src_w, src_h, bpp, fbW, fbH, ss, tables, sdr, groups_x, groups)) return (int)hipErrorInvalidValue;
    const size_t hiW = (size_t)fbW * ss, hiH = (size_t)fbH * 2 * ss;
    const int32_t *tx0 = reinterpret_cast<const int32_t *>(tables);
    const float *twx = reinterpret_cast<const float *>(tables) + hiW;
    const int32_t *ty0 = tx0 + 7 * hiW;
    const float *twy = twx + 6 * hiW + hiH;
    const float inv = 1.0f / (float)(ss * ss);          // :126
    hipLaunchKernelGGL(k_video_blit, dim3(groups), dim3(kVideoBlock), 0, stream, frame, src_w, src_h, bpp, (uint32_t)fbW, ss, groups_x, tx0, twx, ty0, twy, inv, sdr);
    return (int)hipGetLastError();
}

// the quadrant form: ss even; quad_sdr: fbW * fbH * 12 floats {TL rgb, TR rgb, BL rgb, BR rgb}, each the sum of its ss / 2 columns by ss rows
// times 1 / (ss / 2 * ss), saturated; sdr as above, bit for bit
extern "C" int ycge_launch_video_blit_quadrants(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, float *sdr,
                                                float *quad_sdr, hipStream_t stream)
{
    uint32_t groups_x = 0, groups = 0;
    if (!quad_sdr || ss < 2 || (ss & 1) || !video_launch_shape(frame, src_w, src_h, bpp, fbW, fbH, ss, tables, sdr, groups_x, groups)) return (int)hipErrorInvalidValue;
    const size_t hiW = (size_t)fbW * ss, hiH = (size_t)fbH * 2 * ss;
    const int32_t *tx0 = reinterpret_cast<const int32_t *>(tables);
    const float *twx = reinterpret_cast<const float *>(tables) + hiW;
    const int32_t *ty0 = tx0 + 7 * hiW;
    const float *twy = twx + 6 * hiW + hiH;
    const float inv = 1.0f / (float)(ss * ss);
    const float inv_quad = 1.0f / (float)((ss / 2) * ss);
    hipLaunchKernelGGL(k_video_blit_quadrants, dim3(groups), dim3(kVideoBlock), 0, stream, frame, src_w, src_h, bpp, (uint32_t)fbW, ss, groups_x, tx0, twx, ty0, twy, inv,
                       sdr, inv_quad, quad_sdr);
    return (int)hipGetLastError();
}

// k_video_pixels: frame and tables as above, srgb_tables the 256 f32 thresholds of LinearToSrgb8; rgba hiW * hiH words (4-byte aligned), index
// hiW * hiH bytes, either may be NULL, not both
extern "C" int ycge_launch_video_pixels(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, const uint8_t *srgb_tables,
                                        int dither, uint8_t *rgba, uint8_t *index, hipStream_t stream)
{
    uint32_t groups_x = 0, groups = 0;
    const float *some = reinterpret_cast<const float *>(tables);          // (video_launch_shape's sdr: not this launch's)
    if (!video_launch_shape(frame, src_w, src_h, bpp, fbW, fbH, ss, tables, some, groups_x, groups) || !srgb_tables || (!rgba && !index) || ((uintptr_t)rgba & 3u) ||
        dither < 0 || dither > 1)
        return (int)hipErrorInvalidValue;
    const uint64_t hiW = (uint64_t)fbW * ss, hiH = (uint64_t)fbH * 2 * ss;
    if (hiW * hiH > (uint64_t)INT32_MAX / 2) return (int)hipErrorInvalidValue;
    const uint32_t chunks_x = (uint32_t)((hiW + 63u) / 64u);
    const uint64_t chunks = (uint64_t)chunks_x * hiH;
    if (chunks > (uint64_t)INT32_MAX) return (int)hipErrorInvalidValue;
    const int32_t *tx0 = reinterpret_cast<const int32_t *>(tables);
    const float *twx = reinterpret_cast<const float *>(tables) + hiW;
    const int32_t *ty0 = tx0 + 7 * hiW;
    const float *twy = twx + 6 * hiW + hiH;
    const dim3 grid((uint32_t)((chunks + kPixelsBlock / 64 - 1) / (kPixelsBlock / 64))), block(kPixelsBlock);
    uint32_t *r32 = reinterpret_cast<uint32_t *>(rgba);
    if (dither) hipLaunchKernelGGL(k_video_pixels<true>, grid, block, 0, stream, frame, src_w, src_h, bpp, (uint32_t)hiW, chunks_x, (uint32_t)chunks, tx0, twx, ty0, twy, srgb_tables, r32, index);
    else hipLaunchKernelGGL(k_video_pixels<false>, grid, block, 0, stream, frame, src_w, src_h, bpp, (uint32_t)hiW, chunks_x, (uint32_t)chunks, tx0, twx, ty0, twy, srgb_tables, r32, index);
    return (int)hipGetLastError();
}
