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
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace {

constexpr int kVideoBlock = 64;

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
        const int y0 = ty0[y];
        float wy[6];
        uint32_t row[6];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            wy[j] = twy[(size_t)y * 6 + j];
            const int iy = y0 - 2 + j;
            row[j] = (uint32_t)(iy < 0 ? 0 : (iy > src_h - 1 ? src_h - 1 : iy)) * pitch;
        }
#pragma unroll
        for (int h = 0; h < kHalves; h++) {
            for (int sx = h * span; sx < (h + 1) * span; sx++) {
                const uint32_t x = cx * (uint32_t)ss + (uint32_t)sx;
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
                r = clamp01(r); g = clamp01(g); b = clamp01(b);
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
