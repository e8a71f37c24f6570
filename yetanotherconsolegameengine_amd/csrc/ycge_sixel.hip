// ycge_sixel.hip - the sixel presenter's kernels (host side: ycge_sixel.cpp; the contract: include/ycge.h at ycge_render_frame_sixel).
//
// The pixel stage, k_sixel_pixels: one lane maps four consecutive hi-res samples of the denoised buffer (map_pixel of ycge_tonemap.hip.h, no
// box sum), takes their sRGB8 bytes (srgb8 of ycge_srgb8.hip.h over the host's thresholds) and quantises each byte to a level of the
// 6 x 6 x 6 cube: the register plane, one byte a pixel, and the RGBA plane where asked.
//
// The encoder works from the register plane alone, W x H bytes of values below 216, in five launches:
//   k_sixel_presence   per (band, colour) the column of its last pixel + 1 (0: absent), by LDS atomics a column tile, then global ones
//   k_sixel_lines      the compact list of (band, colour) lines, band-major and colour-ascending, and how many there are
//   k_sixel_walk<0>    one wavefront a line: its byte count
//   k_sixel_scan       the exclusive scan of the counts: every line's offset, the header, the trailer, the stream's length
//   k_sixel_walk<1>    the same walk writes the bytes
// The adaptive palette's streams (ycge_sixel_palette.hip) run the PAL instances of presence, lines and walk - 256 registers a band - and
// k_sixel_scan_palette, which takes the length of the register definitions from a device word.
// The delta stream (the contract: include/ycge.h at ycge_render_frame_sixel_delta) is the same five launches in their DELTA instances behind
// k_sixel_diff, which gives every band the span of columns in which it differs from the plane the terminal shows: presence and the walk keep
// to the span, the separators in front of a line count the unchanged bands it skips.  The full stream's instances are what they were.
// The walk takes 64 columns a trip.  Lane x holds the sixel of column x; a lane whose sixel differs from its left neighbour's closes the run
// that ended there (column `width`, one past the colour's last pixel, closes the last one: the empty tail is never walked).  The ballot of
// those lanes gives each its run's first column by a bit scan, the run open at a trip's end is carried in a scalar, and a wavefront prefix
// sum of the runs' byte counts places every run in the line.  Offsets are 32-bit: the host refuses geometries whose bound is not.
// Its own translation unit: the code objects of the other kernels stay what they were.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_sixel_quantise.hip.h"
#include "ycge_srgb8.hip.h"
#include "ycge_tonemap.hip.h"

namespace {

constexpr int kSixelBlock = 256;
// the cube's 216 registers, or (PAL, the adaptive palette of ycge_sixel_palette.hip) up to 256: the second set of the encoder's instances
template <bool PAL> __host__ __device__ constexpr uint32_t registers() { return PAL ? 256u : 216u; }
constexpr uint32_t kPresenceTile = 1024;          // columns a workgroup of k_sixel_presence takes

// one sample: its sRGB8 bytes and its register (the bytes-to-word-and-register tail: ycge_sixel_quantise.hip.h, k_video_pixels' too)
template <bool DITHER>
__device__ __forceinline__ void pixel(ycge::F3 hdr, float exposure, float gamma, float saturation, float vibrance, const float *t32, uint32_t x, uint32_t y,
                                      uint32_t &rgba, uint32_t &reg)
{
    const ycge::F3 m = ycge::map_pixel(hdr, exposure, gamma, saturation, vibrance);
    ycge_sixel::word_and_register<DITHER>(ycge_chexel::clamp01(m.x), ycge_chexel::clamp01(m.y), ycge_chexel::clamp01(m.z), t32, x, y, rgba, reg);
}

// n = W * H samples, rows of W packed (the hi-res buffer's own layout): lane j takes samples 4 j .. 4 j + 3, whichever rows they lie in, so
// that its loads are three float4, its register store one word and its RGBA store one uint4.  The last lane of an n that is no multiple of
// 4 works sample by sample.  Either output may be NULL
template <bool DITHER>
__global__ __launch_bounds__(kSixelBlock) void k_sixel_pixels(const float *__restrict__ hdr, uint32_t W, uint32_t n, float gamma, float saturation, float vibrance,
                                                              const ycge::ToneState *__restrict__ state, const uint8_t *__restrict__ tables,
                                                              uint32_t *__restrict__ rgba_out, uint8_t *__restrict__ index_out)
{
    __shared__ float t32[256];
    t32[threadIdx.x] = reinterpret_cast<const float *>(tables)[threadIdx.x];
    __syncthreads();
    const float exposure = state->effective;
    const uint32_t quads = (n + 3u) / 4u, stride = gridDim.x * kSixelBlock;
    for (uint32_t j = blockIdx.x * kSixelBlock + threadIdx.x; j < quads; j += stride) {
        const uint32_t p0 = 4u * j;
        const uint32_t count = n - p0 < 4u ? n - p0 : 4u;
        float v[12];
        if (count == 4u) {
            const float4 *q = reinterpret_cast<const float4 *>(hdr + (size_t)p0 * 3);
            const float4 a = q[0], b = q[1], c = q[2];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 12; k++) v[k] = k < 3u * count ? hdr[(size_t)p0 * 3 + k] : 0.0f;
        }
        uint32_t y = p0 / W, x = p0 - y * W;
        uint32_t word[4], reg[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            pixel<DITHER>(ycge::f3(v[3 * k], v[3 * k + 1], v[3 * k + 2]), exposure, gamma, saturation, vibrance, t32, x, y, word[k], reg[k]);
            if (++x == W) { x = 0; y++; }
        }
        if (count == 4u) {
            if (rgba_out) reinterpret_cast<uint4 *>(rgba_out)[j] = make_uint4(word[0], word[1], word[2], word[3]);
            if (index_out) reinterpret_cast<uint32_t *>(index_out)[j] = reg[0] | reg[1] << 8 | reg[2] << 16 | reg[3] << 24;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                if (k >= count) continue;
                if (rgba_out) rgba_out[p0 + k] = word[k];
                if (index_out) index_out[p0 + k] = (uint8_t)reg[k];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ the encoder

__device__ __forceinline__ uint32_t digits(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) +
           (v >= 1000000000u);
}

// decimal digits, as put_int of ycge_ansi_cells.hip.h writes them, every store under the capacity
__device__ __forceinline__ uint32_t put_int(uint8_t *s, uint32_t cap, uint32_t p, uint32_t v)
{
    const uint32_t d = digits(v);
    for (uint32_t k = d; k-- > 0; v /= 10u)
        if (p + k < cap) s[p + k] = (uint8_t)('0' + v % 10u);
    return p + d;
}

// The delta stream's spans: span[band] = the smallest column in which any row of the band differs between prev and cur, span[n_bands + band] =
// the largest such column + 1 (0xffffffff and 0 before the launch, and behind it for a band that did not change).  A workgroup takes
// kPresenceTile columns of one band: a lane's columns' minimum and maximum, the wavefronts' by shuffles, the workgroup's in LDS, then at
// most one atomicMin and one atomicMax a workgroup
__global__ __launch_bounds__(kSixelBlock) void k_sixel_diff(const uint8_t *__restrict__ prev, const uint8_t *__restrict__ cur, uint32_t W, uint32_t H,
                                                            uint32_t *__restrict__ span)
{
    __shared__ uint32_t s_lo[kSixelBlock / 64], s_hi[kSixelBlock / 64];
    const uint32_t band = blockIdx.y, x0 = blockIdx.x * kPresenceTile;
    const uint32_t x1 = x0 + kPresenceTile < W ? x0 + kPresenceTile : W;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (uint32_t x = x0 + threadIdx.x; x < x1; x += kSixelBlock) {
        bool differs = false;
#pragma unroll
        for (uint32_t r = 0; r < 6; r++) {
            const uint32_t y = band * 6u + r;
            if (y >= H) break;
            differs |= prev[(size_t)y * W + x] != cur[(size_t)y * W + x];
        }
        if (differs) { lo = lo < x ? lo : x; hi = x + 1u; }          // (a lane's columns ascend)
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t l = __shfl_xor(lo, d, 64), h = __shfl_xor(hi, d, 64);
        lo = l < lo ? l : lo; hi = h > hi ? h : hi;
    }
    if ((threadIdx.x & 63u) == 0u) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kSixelBlock / 64; w++) { lo = s_lo[w] < lo ? s_lo[w] : lo; hi = s_hi[w] > hi ? s_hi[w] : hi; }
        if (hi) { atomicMin(&span[band], lo); atomicMax(&span[gridDim.y + band], hi); }
    }
}

// last1[band * 216 + c]: the column of the last pixel of register c in the band, plus 1 (zero before the launch).  A workgroup takes
// kPresenceTile columns of one band: the tile's maxima in LDS, then one global atomic a colour present.  DELTA: of the band's span alone -
// a register the band holds only outside its span gets no line, an unchanged band none at all
template <bool DELTA, bool PAL>
__global__ __launch_bounds__(kSixelBlock) void k_sixel_presence(const uint8_t *__restrict__ index, uint32_t W, uint32_t H, uint32_t *__restrict__ last1,
                                                                const uint32_t *__restrict__ span)
{
    constexpr uint32_t kRegisters = registers<PAL>();
    __shared__ uint32_t s_last[kRegisters];
    if (threadIdx.x < kRegisters) s_last[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t band = blockIdx.y;
    uint32_t x0 = blockIdx.x * kPresenceTile;
    uint32_t x1 = x0 + kPresenceTile < W ? x0 + kPresenceTile : W;
    if (DELTA) {
        const uint32_t lo = span[band], hi = span[gridDim.y + band];          // (unchanged: lo > hi = 0, no column)
        x0 = x0 > lo ? x0 : lo; x1 = x1 < hi ? x1 : hi;
    }
    for (uint32_t x = x0 + threadIdx.x; x < x1; x += kSixelBlock) {
        uint32_t before = kRegisters;
#pragma unroll
        for (uint32_t r = 0; r < 6; r++) {
            const uint32_t y = band * 6u + r;
            if (y >= H) break;
            const uint32_t c = index[(size_t)y * W + x];
            if (c != before && c < kRegisters) atomicMax(&s_last[c], x + 1u);
            before = c;
        }
    }
    __syncthreads();
    if (threadIdx.x < kRegisters && s_last[threadIdx.x]) atomicMax(&last1[(size_t)band * kRegisters + threadIdx.x], s_last[threadIdx.x]);
}

// exclusive scan of one value per lane over the workgroup (the form of ycge_ansi_cells.hip.h); total: the sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kSixelBlock / 64; w++) {
        const uint32_t s = wsum[w];
        before += w < wid ? s : 0u;
        total += s;
    }
    __syncthreads();                      // (wsum may be reused)
    return before + inc - v;
}

// one workgroup: lines[] = band << 8 | colour for every colour present, band-major and colour-ascending; meta[0] = how many.  A lane takes a
// band: its place is the scan of the bands' counts
template <bool PAL>
__global__ __launch_bounds__(kSixelBlock) void k_sixel_lines(const uint32_t *__restrict__ last1, uint32_t n_bands, uint32_t max_lines, uint32_t *__restrict__ lines,
                                                             uint32_t *__restrict__ meta)
{
    constexpr uint32_t kRegisters = registers<PAL>();
    __shared__ uint32_t wsum[kSixelBlock / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_bands; base += kSixelBlock) {
        const uint32_t band = base + threadIdx.x;
        uint32_t mine = 0;
        if (band < n_bands)
            for (uint32_t c = 0; c < kRegisters; c++) mine += last1[(size_t)band * kRegisters + c] != 0u;
        uint32_t total;
        uint32_t at = carry + block_exclusive_scan(mine, wsum, total);
        if (band < n_bands)
            for (uint32_t c = 0; c < kRegisters; c++)
                if (last1[(size_t)band * kRegisters + c] != 0u) {
                    if (at < max_lines) lines[at] = band << 8 | c;
                    at++;
                }
        carry += total;
    }
    if (threadIdx.x == 0) meta[0] = carry < max_lines ? carry : max_lines;
}

// One wavefront a line, grid-stride over the meta[0] lines.  WRITE = false: line_bytes[line] = the line's bytes - '#', the register's digits,
// the runs, and the separator behind it ('$' inside a band, '-' behind a band's last line, none behind the stream's last line).
// WRITE = true: the same bytes at line_bytes[line], which the scan made the line's offset.
// DELTA: the line's sixels are zero left of its band's span[band] - the trips in front of that column's are not walked, the run of empty
// columns opens at column 0 all the same - and its separators stand IN FRONT of it: '$' behind a line of the same band, else one '-' for
// every band between the line before (the stream's first line: band 0) and its own, unchanged bands included; none behind the last line
template <bool WRITE, bool DELTA, bool PAL>
__global__ __launch_bounds__(kSixelBlock) void k_sixel_walk(const uint8_t *__restrict__ index, uint32_t W, uint32_t H, const uint32_t *__restrict__ last1,
                                                            const uint32_t *__restrict__ lines, const uint32_t *__restrict__ meta,
                                                            uint32_t *__restrict__ line_bytes, uint8_t *__restrict__ out, uint32_t cap,
                                                            const uint32_t *__restrict__ span)
{
    constexpr uint32_t kRegisters = registers<PAL>();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_lines = meta[0];
    const uint32_t waves = gridDim.x * (kSixelBlock / 64);
    for (uint32_t line = blockIdx.x * (kSixelBlock / 64) + (threadIdx.x >> 6); line < n_lines; line += waves) {
        const uint32_t key = lines[line], band = key >> 8, colour = key & 0xffu;
        const uint32_t width = last1[(size_t)band * kRegisters + colour];          // columns 0 .. width - 1 are walked; >= 1 and <= W
        const uint32_t rows = H - band * 6u < 6u ? H - band * 6u : 6u;
        const uint8_t *row0 = index + (size_t)band * 6u * W;
        uint32_t at = WRITE ? line_bytes[line] : 0u;                                // where the next byte goes (WRITE) / the bytes so far
        uint32_t lo = 0;
        if (DELTA) {
            lo = span[band];
            const uint32_t before = line ? lines[line - 1u] >> 8 : 0u;
            const uint32_t lead = line && before == band ? 1u : band - before;    // '$', or the '-' of every band from `before` to this one
            if (WRITE)
                for (uint32_t k = lane; k < lead; k += 64u)
                    if (at + k < cap) out[at + k] = (uint8_t)(line && before == band ? '$' : '-');
            at += lead;
        }
        if (WRITE) {
            if (lane == 0) {
                if (at < cap) out[at] = (uint8_t)'#';
                (void)put_int(out, cap, at + 1u, colour);
            }
        }
        at += 1u + digits(colour);
        uint32_t run_first = 0, left_carry = 0;                                    // the open run's first column; the sixel of the column before this trip
        for (uint32_t base = DELTA ? lo & ~63u : 0u; base <= width; base += 64u) {
            const uint32_t x = base + lane;
            uint32_t six = 0x80u;                                                  // column `width` and beyond: no sixel's value
            if (x < width) {
                six = 0;
                if (!DELTA || x >= lo)
                for (uint32_t r = 0; r < rows; r++) six |= (uint32_t)(row0[(size_t)r * W + x] == colour) << r;
            }
            uint32_t left = __shfl_up(six, 1, 64);
            if (lane == 0) left = left_carry;
            const bool closes = x >= 1u && x <= width && six != left;              // the run of `left` ended at column x - 1
            const unsigned long long mask = __ballot(closes);
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            const uint32_t first = below ? base + 63u - (uint32_t)__clzll((long long)below) : run_first;
            const uint32_t n = x - first;
            const uint32_t bytes = closes ? (n >= 4u ? 2u + digits(n) : n) : 0u;
            uint32_t inc = bytes;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t u = __shfl_up(inc, d, 64);
                if (lane >= (uint32_t)d) inc += u;
            }
            if (WRITE && closes) {
                uint32_t p = at + inc - bytes;
                const uint8_t ch = (uint8_t)(63u + left);
                if (n >= 4u) {
                    if (p < cap) out[p] = (uint8_t)'!';
                    p = put_int(out, cap, p + 1u, n);
                    if (p < cap) out[p] = ch;
                } else {
                    for (uint32_t k = 0; k < n; k++)
                        if (p + k < cap) out[p + k] = ch;
                }
            }
            at += __shfl(inc, 63, 64);
            if (mask) run_first = base + 63u - (uint32_t)__clzll((long long)mask);
            left_carry = __shfl(six, 63, 64);
        }
        // the separator: none behind the last line of the stream
        if (DELTA) {
            if (!WRITE && lane == 0) line_bytes[line] = at;
            continue;
        }
        const bool last_line = line + 1u == n_lines;
        const bool band_ends = last_line || (lines[line + 1u] >> 8) != band;
        if (WRITE) {
            if (lane == 0 && !last_line && at < cap) out[at] = (uint8_t)(band_ends ? '-' : '$');
        } else if (lane == 0) {
            line_bytes[line] = at + (last_line ? 0u : 1u);
        }
    }
}

// one workgroup: the lines' byte counts -> their offsets in place, behind the header; the header's bytes and the trailer ESC \ into the
// stream; res[0] = the stream's length.  DELTA: and res[1..3] = the changed bands, the pixels painted (span width x band rows, summed) and the lines
template <bool DELTA>
__global__ __launch_bounds__(kSixelBlock) void k_sixel_scan(uint32_t *__restrict__ line_bytes, const uint32_t *__restrict__ meta, const uint8_t *__restrict__ header,
                                                            uint32_t header_bytes, uint8_t *__restrict__ out, uint32_t cap, unsigned long long *__restrict__ res,
                                                            const uint32_t *__restrict__ span, uint32_t n_bands, uint32_t H)
{
    __shared__ uint32_t wsum[kSixelBlock / 64];
    const uint32_t n_lines = meta[0];
    unsigned long long carry = header_bytes;
    for (uint32_t base = 0; base < n_lines; base += kSixelBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_lines ? line_bytes[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, total);
        if (t < n_lines) line_bytes[t] = (uint32_t)carry + ex;
        carry += total;
    }
    for (uint32_t k = threadIdx.x; k < header_bytes; k += kSixelBlock)
        if (k < cap) out[k] = header[k];
    if (threadIdx.x < 2 && carry + threadIdx.x < cap) out[carry + threadIdx.x] = (uint8_t)"\x1b\\"[threadIdx.x];
    if (threadIdx.x == 0) res[0] = carry + 2ull;
    if (DELTA) {
        __shared__ unsigned long long s_info[2];
        if (threadIdx.x < 2) s_info[threadIdx.x] = 0ull;
        __syncthreads();
        unsigned long long changed = 0, painted = 0;
        for (uint32_t band = threadIdx.x; band < n_bands; band += kSixelBlock) {
            const uint32_t lo = span[band], hi = span[n_bands + band];
            if (!hi) continue;
            const uint32_t rows = H - band * 6u < 6u ? H - band * 6u : 6u;
            changed++; painted += (unsigned long long)(hi - lo) * rows;
        }
        if (changed) { atomicAdd(&s_info[0], changed); atomicAdd(&s_info[1], painted); }
        __syncthreads();
        if (threadIdx.x == 0) { res[1] = s_info[0]; res[2] = s_info[1]; res[3] = n_lines; }
    }
}

// k_sixel_scan<false> for the adaptive palette's stream: the header is the host's prefix (parts 1 to 4) and behind it the register
// definitions k_pal_build wrote on the device, *defs_bytes of them - the host never learns the header's length before the stream's
__global__ __launch_bounds__(kSixelBlock) void k_sixel_scan_palette(uint32_t *__restrict__ line_bytes, const uint32_t *__restrict__ meta, const uint8_t *__restrict__ prefix,
                                                                    uint32_t prefix_bytes, const uint8_t *__restrict__ defs, const uint32_t *__restrict__ defs_bytes,
                                                                    uint8_t *__restrict__ out, uint32_t cap, unsigned long long *__restrict__ res)
{
    __shared__ uint32_t wsum[kSixelBlock / 64];
    const uint32_t n_lines = meta[0], n_defs = defs_bytes[0];
    unsigned long long carry = (unsigned long long)prefix_bytes + n_defs;
    for (uint32_t base = 0; base < n_lines; base += kSixelBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_lines ? line_bytes[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, total);
        if (t < n_lines) line_bytes[t] = (uint32_t)carry + ex;
        carry += total;
    }
    for (uint32_t k = threadIdx.x; k < prefix_bytes; k += kSixelBlock)
        if (k < cap) out[k] = prefix[k];
    for (uint32_t k = threadIdx.x; k < n_defs; k += kSixelBlock)
        if (prefix_bytes + k < cap) out[prefix_bytes + k] = defs[k];
    if (threadIdx.x < 2 && carry + threadIdx.x < cap) out[carry + threadIdx.x] = (uint8_t)"\x1b\\"[threadIdx.x];
    if (threadIdx.x == 0) res[0] = carry + 2ull;
}

} // namespace

extern "C" {

// k_sixel_pixels over a hi-res buffer of W x H samples, rows packed (16-byte aligned): rgba W*H words (16-byte aligned), index W*H bytes
// (4-byte aligned); either may be NULL, not both.  state: the tone state whose effective exposure maps the frame
int ycge_launch_sixel_pixels(const float *hdr, int W, int H, float gamma, float saturation, float vibrance, const void *state, const uint8_t *tables, int dither,
                             uint8_t *rgba, uint8_t *index, int compute_units, hipStream_t stream)
{
    if (!hdr || !state || !tables || (!rgba && !index) || W <= 0 || H <= 0 || (int64_t)W * H > (int64_t)INT32_MAX / 2 || ((uintptr_t)hdr & 15u) ||
        ((uintptr_t)rgba & 15u) || ((uintptr_t)index & 3u) || dither < 0 || dither > 1)
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t need = ((n + 3u) / 4u + kSixelBlock - 1) / kSixelBlock;
    const uint32_t cap = (uint32_t)(compute_units > 0 ? compute_units : 256) * 8u;
    const dim3 grid(need < cap ? need : cap), block(kSixelBlock);
    const ycge::ToneState *ts = static_cast<const ycge::ToneState *>(state);
    uint32_t *r32 = reinterpret_cast<uint32_t *>(rgba);
    if (dither) hipLaunchKernelGGL(k_sixel_pixels<true>, grid, block, 0, stream, hdr, (uint32_t)W, n, gamma, saturation, vibrance, ts, tables, r32, index);
    else hipLaunchKernelGGL(k_sixel_pixels<false>, grid, block, 0, stream, hdr, (uint32_t)W, n, gamma, saturation, vibrance, ts, tables, r32, index);
    return (int)hipGetLastError();
}

// The encoder on a register plane of W x H bytes.  last1: n_bands * 216 words; lines and line_bytes: max_lines words each, max_lines >=
// n_bands * min(216, 6 W); meta: 1 word; header: the stream's parts 1 to 5; out: cap bytes; res: 1 word of 64 bits, the length
// prev and span (both or neither): the delta stream against the plane prev - span: 2 * n_bands words, header: the delta's, res: 4 words of 64
// bits {length, changed bands, pixels painted, lines}
int ycge_launch_sixel_encode(const uint8_t *index, int W, int H, uint32_t *last1, uint32_t *lines, uint32_t *line_bytes, uint32_t max_lines, uint32_t *meta,
                             const uint8_t *header, uint32_t header_bytes, uint8_t *out, uint32_t cap, unsigned long long *res, int compute_units, hipStream_t stream,
                             const uint8_t *prev, uint32_t *span)
{
    if ((prev != nullptr) != (span != nullptr)) return (int)hipErrorInvalidValue;
    if (!index || !last1 || !lines || !line_bytes || !meta || !header || !out || !res || W <= 0 || H <= 0 || H > (1 << 24)) return (int)hipErrorInvalidValue;
    const uint32_t n_bands = ((uint32_t)H + 5u) / 6u;
    constexpr uint32_t kRegisters = registers<false>();
    const uint64_t colours = 6ull * (uint32_t)W < kRegisters ? 6ull * (uint32_t)W : kRegisters;
    if ((uint64_t)n_bands * colours > max_lines || n_bands > 65535u) return (int)hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(last1, 0, (size_t)n_bands * kRegisters * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
    const dim3 tiles(((uint32_t)W + kPresenceTile - 1) / kPresenceTile, n_bands);
    if (prev) {
        e = hipMemsetAsync(span, 0xff, (size_t)n_bands * sizeof(uint32_t), stream);
        if (e == hipSuccess) e = hipMemsetAsync(span + n_bands, 0, (size_t)n_bands * sizeof(uint32_t), stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_sixel_diff, tiles, dim3(kSixelBlock), 0, stream, prev, index, (uint32_t)W, (uint32_t)H, span);
        hipLaunchKernelGGL((k_sixel_presence<true, false>), tiles, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, span);
    } else {
        hipLaunchKernelGGL((k_sixel_presence<false, false>), tiles, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, span);
    }
    hipLaunchKernelGGL(k_sixel_lines<false>, dim3(1), dim3(kSixelBlock), 0, stream, last1, n_bands, max_lines, lines, meta);
    const uint32_t need = (max_lines + kSixelBlock / 64 - 1) / (kSixelBlock / 64);
    const uint32_t limit = (uint32_t)(compute_units > 0 ? compute_units : 256) * 8u;
    const dim3 grid(need < limit ? need : limit);
    if (prev) {
        hipLaunchKernelGGL((k_sixel_walk<false, true, false>), grid, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, lines, meta, line_bytes, out, cap, span);
        hipLaunchKernelGGL(k_sixel_scan<true>, dim3(1), dim3(kSixelBlock), 0, stream, line_bytes, meta, header, header_bytes, out, cap, res, span, n_bands, (uint32_t)H);
        hipLaunchKernelGGL((k_sixel_walk<true, true, false>), grid, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, lines, meta, line_bytes, out, cap, span);
    } else {
        hipLaunchKernelGGL((k_sixel_walk<false, false, false>), grid, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, lines, meta, line_bytes, out, cap, span);
        hipLaunchKernelGGL(k_sixel_scan<false>, dim3(1), dim3(kSixelBlock), 0, stream, line_bytes, meta, header, header_bytes, out, cap, res, span, n_bands, (uint32_t)H);
        hipLaunchKernelGGL((k_sixel_walk<true, false, false>), grid, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, lines, meta, line_bytes, out, cap, span);
    }
    return (int)hipGetLastError();
}

// The encoder's PAL instances on a register plane of the adaptive palette (values below 256; the full stream alone).  last1: n_bands * 256
// words; max_lines >= n_bands * min(256, 6 W); prefix: the stream's parts 1 to 4; defs / defs_bytes: the definitions and their length on the
// device; res: 1 word of 64 bits, the length
int ycge_launch_sixel_encode_palette(const uint8_t *index, int W, int H, uint32_t *last1, uint32_t *lines, uint32_t *line_bytes, uint32_t max_lines, uint32_t *meta,
                                     const uint8_t *prefix, uint32_t prefix_bytes, const uint8_t *defs, const uint32_t *defs_bytes, uint8_t *out, uint32_t cap,
                                     unsigned long long *res, int compute_units, hipStream_t stream)
{
    if (!index || !last1 || !lines || !line_bytes || !meta || !prefix || !defs || !defs_bytes || !out || !res || W <= 0 || H <= 0 || H > (1 << 24)) return (int)hipErrorInvalidValue;
    constexpr uint32_t kRegisters = registers<true>();
    const uint32_t n_bands = ((uint32_t)H + 5u) / 6u;
    const uint64_t colours = 6ull * (uint32_t)W < kRegisters ? 6ull * (uint32_t)W : kRegisters;
    if ((uint64_t)n_bands * colours > max_lines || n_bands > 65535u) return (int)hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(last1, 0, (size_t)n_bands * kRegisters * sizeof(uint32_t), stream);
    if (e != hipSuccess) return (int)e;
    const dim3 tiles(((uint32_t)W + kPresenceTile - 1) / kPresenceTile, n_bands);
    hipLaunchKernelGGL((k_sixel_presence<false, true>), tiles, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, (const uint32_t *)nullptr);
    hipLaunchKernelGGL(k_sixel_lines<true>, dim3(1), dim3(kSixelBlock), 0, stream, last1, n_bands, max_lines, lines, meta);
    const uint32_t need = (max_lines + kSixelBlock / 64 - 1) / (kSixelBlock / 64);
    const uint32_t limit = (uint32_t)(compute_units > 0 ? compute_units : 256) * 8u;
    const dim3 grid(need < limit ? need : limit);
    hipLaunchKernelGGL((k_sixel_walk<false, false, true>), grid, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, lines, meta, line_bytes, out, cap,
                       (const uint32_t *)nullptr);
    hipLaunchKernelGGL(k_sixel_scan_palette, dim3(1), dim3(kSixelBlock), 0, stream, line_bytes, meta, prefix, prefix_bytes, defs, defs_bytes, out, cap, res);
    hipLaunchKernelGGL((k_sixel_walk<true, false, true>), grid, dim3(kSixelBlock), 0, stream, index, (uint32_t)W, (uint32_t)H, last1, lines, meta, line_bytes, out, cap,
                       (const uint32_t *)nullptr);
    return (int)hipGetLastError();
}

} // extern "C"
