// ycge_chexel.hip - the presenters' colour maps on the device (host side: ycge_chexel.cpp).
//
// One lane per chexel reads the frame's SDR {top rgb, bottom rgb} (what k_tonemap_downsample wrote) and writes the bytes a presenter
// consumes, each only where asked:
//   c16  - ChexelColor(Vec3).color_16 of top | of bottom << 4 (Chexel.cs:37-41, 70-99): the low byte of Win32's MapAttributes(fg, bg)
//   ansi - ChexelToAnsi256 of top, of bottom (ANSITerminalRenderer.cs:246-306)
//   rgba - OpenGLTerminalRenderer's compose image (:114-145, LinearToSrgb8 :390-400): fbW x 2 fbH RGBA8, row 2 cy the top half-cell
// Its own translation unit, as ycge_query.hip is: the code objects of the frame kernels stay what they were.
//
// LinearToSrgb8 is a monotone step function of its input; no byte is decided by a device pow.  The host computed its 255 thresholds
// once with the C library's double pow (ycge_chexel.cpp): t32[k - 1] is the smallest binary32 and t64[k - 1] the smallest binary64
// whose byte is >= k, so the byte is the number of thresholds <= x - NaN and negatives count none, values above 1 count all 255.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "ycge_srgb8.hip.h"

namespace {

constexpr int kChexelBlock = 256;

// Chexel.cs:11-29, component by component (0 0.5 0.75 1 are exact in binary32)
__constant__ float c_palette16[16][3] = {
    {0.00f, 0.00f, 0.00f}, {0.00f, 0.00f, 0.50f}, {0.00f, 0.50f, 0.00f}, {0.00f, 0.50f, 0.50f},
    {0.50f, 0.00f, 0.00f}, {0.50f, 0.00f, 0.50f}, {0.50f, 0.50f, 0.00f}, {0.75f, 0.75f, 0.75f},
    {0.50f, 0.50f, 0.50f}, {0.00f, 0.00f, 1.00f}, {0.00f, 1.00f, 0.00f}, {0.00f, 1.00f, 1.00f},
    {1.00f, 0.00f, 0.00f}, {1.00f, 0.00f, 1.00f}, {1.00f, 1.00f, 0.00f}, {1.00f, 1.00f, 1.00f}};

using ycge_chexel::clamp01;          // Clamp01 (Chexel.cs:92-98) and the threshold search: ycge_srgb8.hip.h
using ycge_chexel::srgb8;

// NearestConsoleColorFrom (Chexel.cs:70-89) on clamped channels: binary32 distances left to right, strict <, ties to the lower index
__device__ __forceinline__ uint32_t color16(float r, float g, float b)
{
    uint32_t best = 0;
    float best_d = FLT_MAX;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float dr = r - c_palette16[i][0], dg = g - c_palette16[i][1], db = b - c_palette16[i][2];
        const float d = dr * dr + dg * dg + db * db;
        if (d < best_d) { best_d = d; best = (uint32_t)i; }
    }
    return best;
}

// ToCubeLevelSrgb (ANSITerminalRenderer.cs:276-284)
__device__ __forceinline__ int cube_level(int v) { return (v >= 48) + (v >= 114) + (v >= 154) + (v >= 194) + (v >= 234); }

// ChexelToAnsi256 (ANSITerminalRenderer.cs:246-274) of a ChexelColor whose channels are already Clamp01'd; b8 = the three sRGB bytes
__device__ __forceinline__ uint32_t ansi256(float r, float g, float b, const int b8[3], const double *t64)
{
    const int cube_v[6] = {0, 95, 135, 175, 215, 255};
    const int ir = cube_level(b8[0]), ig = cube_level(b8[1]), ib = cube_level(b8[2]);
    const int idx_cube = 16 + 36 * ir + 6 * ig + ib;
    // luminance in double, left to right, on the clamped channels; the clamp is LinearToSrgb8's own (the Clamp01 values pass it)
    const double rl = (double)r, gl = (double)g, bl = (double)b;
    const double y = 0.2126 * rl + 0.7152 * gl + 0.0722 * bl;
    const int y8 = srgb8(t64, y);
    int gray_idx = (int)rint(((double)y8 - 8.0) / 10.0);          // Math.Round: half to even
    gray_idx = gray_idx < 0 ? 0 : (gray_idx > 23 ? 23 : gray_idx);
    // s_graySrgb is allocated and never filled (:26, read at :272): the gray candidate's value is 0, its distance is to black
    const int drg = abs(b8[0] - b8[1]), drb = abs(b8[0] - b8[2]), dgb = abs(b8[1] - b8[2]);
    const int chroma = max(drg, max(drb, dgb));
    const int cr = b8[0] - cube_v[ir], cg = b8[1] - cube_v[ig], cb = b8[2] - cube_v[ib];
    const int d_cube = cr * cr + cg * cg + cb * cb;
    const int d_gray = chroma <= 18 ? b8[0] * b8[0] + b8[1] * b8[1] + b8[2] * b8[2] + 64 : INT32_MAX;
    return (uint32_t)(d_gray < d_cube ? 232 + gray_idx : idx_cube);
}

// one half-cell: r g b as the SDR array holds them -> its console-16 index, ANSI-256 index, RGBA8 word
template <bool SRGB>
__device__ __forceinline__ void half_cell(float r, float g, float b, const float *t32, const double *t64, uint32_t &c16, uint32_t &ansi, uint32_t &rgba)
{
    r = clamp01(r); g = clamp01(g); b = clamp01(b);
    c16 = color16(r, g, b);
    if (SRGB) {
        const int b8[3] = {srgb8(t32, r), srgb8(t32, g), srgb8(t32, b)};
        ansi = ansi256(r, g, b, b8, t64);
        rgba = (uint32_t)b8[0] | (uint32_t)b8[1] << 8 | (uint32_t)b8[2] << 16 | 0xff000000u;
    }
}

// grid-stride over n = fbW * fbH chexels; `tables` = 256 f32 thresholds then 256 f64 ones (entry 255 of each is padding)
template <bool SRGB>
__global__ __launch_bounds__(kChexelBlock) void k_encode_chexels(const float *__restrict__ sdr, uint32_t fbW, uint32_t n, const uint8_t *__restrict__ tables,
                                                                 uint8_t *__restrict__ c16_out, uint16_t *__restrict__ ansi_out, uint32_t *__restrict__ rgba_out)
{
    __shared__ float t32[256];
    __shared__ double t64[256];
    if (SRGB) {
        t32[threadIdx.x] = reinterpret_cast<const float *>(tables)[threadIdx.x];
        t64[threadIdx.x] = reinterpret_cast<const double *>(tables + 1024)[threadIdx.x];
        __syncthreads();
    }
    const uint32_t stride = gridDim.x * kChexelBlock;
    for (uint32_t i = blockIdx.x * kChexelBlock + threadIdx.x; i < n; i += stride) {
        const float2 *p = reinterpret_cast<const float2 *>(sdr + (size_t)i * 6);
        const float2 a = p[0], b = p[1], c = p[2];          // top r g, top b / bottom r, bottom g b
        uint32_t c16t, c16b, at = 0, ab = 0, pt = 0, pb = 0;
        half_cell<SRGB>(a.x, a.y, b.x, t32, t64, c16t, at, pt);
        half_cell<SRGB>(b.y, c.x, c.y, t32, t64, c16b, ab, pb);
        if (c16_out) c16_out[i] = (uint8_t)(c16t | c16b << 4);
        if (SRGB) {
            if (ansi_out) ansi_out[i] = (uint16_t)(at | ab << 8);
            if (rgba_out) {
                const uint32_t cy = i / fbW, cx = i - cy * fbW;
                const size_t top = (size_t)(2 * cy) * fbW + cx;
                rgba_out[top] = pt;
                rgba_out[top + fbW] = pb;
            }
        }
    }
}

// The quadrant-glyph fit (the contract: include/ycge.h at ycge_render_frame_quadrants): one lane a chexel reads its four sub-cell colours
// {TL, TR, BL, BR} (k_tonemap_quadrants), takes their sRGB8 bytes as half_cell does, and picks the quadrant block glyph and the two colours
// that approximate the four with the least squared error.  All integer from the bytes on.  Mask m in 0..7: bit 0 = TL, bit 1 = TR, bit 2 = BL
// in the foreground, BR always background.  With S_F / S_B the channel sums over foreground / background, minimising the error is maximising
// |S_B|^2 / |B| + |S_F|^2 / |F|; w(n) = 12 / n makes that an int32 (below 2^24).  Ties go to the smallest m.
__constant__ uint16_t c_quadrant_glyph[8] = {0x2580, 0x2598, 0x259d, 0x2580, 0x2596, 0x258c, 0x259e, 0x259b};

__global__ __launch_bounds__(kChexelBlock) void k_fit_quadrants(const float *__restrict__ quad, uint32_t fbW, uint32_t n, const uint8_t *__restrict__ tables,
                                                                int32_t min_contrast, uint16_t *__restrict__ glyph_out, uint32_t *__restrict__ rgba_out)
{
    __shared__ float t32[256];
    t32[threadIdx.x] = reinterpret_cast<const float *>(tables)[threadIdx.x];
    __syncthreads();
    const uint32_t stride = gridDim.x * kChexelBlock;
    for (uint32_t i = blockIdx.x * kChexelBlock + threadIdx.x; i < n; i += stride) {
        const float4 *p = reinterpret_cast<const float4 *>(quad + (size_t)i * 12);
        const float4 v0 = p[0], v1 = p[1], v2 = p[2];
        const float x[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
        int q[4][3], s0[3] = {0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int c = 0; c < 3; c++) { q[k][c] = srgb8(t32, clamp01(x[3 * k + c])); s0[c] += q[k][c]; }
        int contrast = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int mean = (2 * s0[c] + 4) / 8;
#pragma unroll
            for (int k = 0; k < 4; k++) contrast = max(contrast, abs(q[k][c] - mean));
        }
        int best = 0;
        if (contrast > min_contrast) {
            int best_score = -1;
#pragma unroll
            for (int m = 0; m < 8; m++) {
                const int nf = (m & 1) + (m >> 1 & 1) + (m >> 2 & 1), nb = 4 - nf;
                int score = 0;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int sf = (m & 1 ? q[0][c] : 0) + (m & 2 ? q[1][c] : 0) + (m & 4 ? q[2][c] : 0), sb = s0[c] - sf;
                    score += (12 / nb) * sb * sb + (nf ? (12 / nf) * sf * sf : 0);
                }
                if (score > best_score) { best_score = score; best = m; }
            }
        }
        const int nf = (best & 1) + (best >> 1 & 1) + (best >> 2 & 1), nb = 4 - nf;
        uint32_t fg = 0, bg = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int sf = (best & 1 ? q[0][c] : 0) + (best & 2 ? q[1][c] : 0) + (best & 4 ? q[2][c] : 0), sb = s0[c] - sf;
            const int b8 = (2 * sb + nb) / (2 * nb), f8 = nf ? (2 * sf + nf) / (2 * nf) : b8;
            fg |= (uint32_t)f8 << (8 * c); bg |= (uint32_t)b8 << (8 * c);
        }
        if (glyph_out) glyph_out[i] = c_quadrant_glyph[best];
        if (rgba_out) {
            const uint32_t cy = i / fbW, cx = i - cy * fbW;
            const size_t top = (size_t)(2 * cy) * fbW + cx;
            rgba_out[top] = fg | 0xff000000u;
            rgba_out[top + fbW] = bg | 0xff000000u;
        }
    }
}

} // namespace

// k_fit_quadrants on the fbW x fbH chexels' sub-cell colours (12 floats a chexel, 16-byte aligned): glyphs fbW*fbH code units, rgba the
// plane of k_encode_chexels' layout, row 2 cy the foreground and row 2 cy + 1 the background; either may be NULL, not both
extern "C" int ycge_launch_quadrant_fit(const float *quad, int fbW, int fbH, const uint8_t *tables, int min_contrast, uint16_t *glyphs, uint8_t *rgba,
                                        int compute_units, hipStream_t stream)
{
    if (fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2 || !quad || ((uintptr_t)quad & 15u) || !tables || (!glyphs && !rgba) ||
        ((uintptr_t)rgba & 3u) || ((uintptr_t)glyphs & 1u) || min_contrast < 0 || min_contrast > 255)
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)fbW * (uint32_t)fbH;
    const uint32_t need = (n + kChexelBlock - 1) / kChexelBlock;
    const uint32_t cap = (uint32_t)(compute_units > 0 ? compute_units : 256) * 8u;
    hipLaunchKernelGGL(k_fit_quadrants, dim3(need < cap ? need : cap), dim3(kChexelBlock), 0, stream, quad, (uint32_t)fbW, n, tables, (int32_t)min_contrast, glyphs,
                       reinterpret_cast<uint32_t *>(rgba));
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_chexels(const float *sdr, int fbW, int fbH, const uint8_t *tables, uint8_t *c16, uint8_t *ansi, uint8_t *rgba,
                                   int compute_units, hipStream_t stream)
{
    if (fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2 || !sdr || (!c16 && !ansi && !rgba) || ((ansi || rgba) && !tables))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)fbW * (uint32_t)fbH;
    const uint32_t need = (n + kChexelBlock - 1) / kChexelBlock;
    const uint32_t cap = (uint32_t)(compute_units > 0 ? compute_units : 256) * 8u;     // 8 workgroups of 256 lanes per CU, then grid stride
    const dim3 grid(need < cap ? need : cap), block(kChexelBlock);
    uint16_t *a16 = reinterpret_cast<uint16_t *>(ansi);
    uint32_t *r32 = reinterpret_cast<uint32_t *>(rgba);
    if (ansi || rgba) hipLaunchKernelGGL(k_encode_chexels<true>, grid, block, 0, stream, sdr, (uint32_t)fbW, n, tables, c16, a16, r32);
    else hipLaunchKernelGGL(k_encode_chexels<false>, grid, block, 0, stream, sdr, (uint32_t)fbW, n, tables, c16, a16, r32);
    return (int)hipGetLastError();
}
