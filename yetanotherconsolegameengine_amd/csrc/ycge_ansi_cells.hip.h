// ycge_ansi_cells.hip.h - what the two ANSI stream units share on the device (ycge_ansi.hip: the full stream, ycge_ansi_delta.hip: the
// delta stream): the tile shape, a console cell's lookup, decimal digits, the byte writers and the workgroup scan.  Everything is inlined
// into the unit that includes it; neither unit's kernels call into the other.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ycge_ansi {

constexpr int kAnsiBlock = 256;
constexpr int kAnsiPerLane = 4;                                   // consecutive cells per lane
constexpr int kAnsiTile = kAnsiBlock * kAnsiPerLane;

struct AnsiArgs {
    const uint8_t *pairs;                 // fbW x fbH {fg = ansi(top), bg = ansi(bottom)}, what k_encode_chexels writes
    const uint8_t *palette;               // ansi(palette16[k]) at byte k (k_encode_chexels on the 16 palette values)
    int32_t fbW, fbH, cw, vx, vy, dfg, dbg;
    uint32_t n;                           // console cells, cw * ch
};

struct Cell {
    uint32_t x, y, fg, bg;
    bool covered;                         // a framebuffer chexel ('▀'); otherwise the default cell (' ')
};

// GetChexelForPoint (:67-84) with the raytrace framebuffer alone: its chexels are '▀', never ' ', so no layer below shows through
__device__ __forceinline__ Cell cell_at(const AnsiArgs &a, uint32_t i)
{
    Cell c;
    c.y = i / (uint32_t)a.cw;
    c.x = i - c.y * (uint32_t)a.cw;
    const int64_t fx = (int64_t)c.x - a.vx, fy = (int64_t)c.y - a.vy;
    c.covered = fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH;
    if (c.covered) {
        const uint8_t *p = a.pairs + 2 * ((size_t)fy * (uint32_t)a.fbW + (size_t)fx);
        c.fg = p[0]; c.bg = p[1];
    } else {
        c.fg = a.palette[a.dfg]; c.bg = a.palette[a.dbg];
    }
    return c;
}

// AppendInt (:181-202) on a non-negative value: its decimal digits, '0' for zero
__device__ __forceinline__ uint32_t digits(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}

// the SGR escape of Render()'s three branches (:120-143) for indices (fg, bg) behind (pfg, pbg) (256: none yet): its length
__device__ __forceinline__ uint32_t sgr_bytes(uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
{
    const bool f = fg != pfg, b = bg != pbg;
    if (f && b) return 14u + digits(fg) + digits(bg);              // ESC [ 3 8 ; 5 ; F ; 4 8 ; 5 ; B m
    if (f) return 8u + digits(fg);                                // ESC [ 3 8 ; 5 ; F m
    if (b) return 8u + digits(bg);                                // ESC [ 4 8 ; 5 ; B m
    return 0u;
}

__device__ __forceinline__ uint32_t put_ascii(uint8_t *s, uint32_t p, const char *t)
{
    for (; *t; t++) s[p++] = (uint8_t)*t;
    return p;
}

__device__ __forceinline__ uint32_t put_int(uint8_t *s, uint32_t p, uint32_t v)
{
    const uint32_t d = digits(v);
    for (uint32_t k = d; k-- > 0; v /= 10u) s[p + k] = (uint8_t)('0' + v % 10u);
    return p + d;
}

// ... and its bytes
__device__ __forceinline__ uint32_t put_sgr(uint8_t *s, uint32_t p, uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
{
    const bool f = fg != pfg, b = bg != pbg;
    if (f && b) { p = put_ascii(s, p, "\x1b[38;5;"); p = put_int(s, p, fg); p = put_ascii(s, p, ";48;5;"); p = put_int(s, p, bg); s[p++] = 'm'; }
    else if (f) { p = put_ascii(s, p, "\x1b[38;5;"); p = put_int(s, p, fg); s[p++] = 'm'; }
    else if (b) { p = put_ascii(s, p, "\x1b[48;5;"); p = put_int(s, p, bg); s[p++] = 'm'; }
    return p;
}

// the cell's character: '▀' U+2580 in UTF-8 when covered, ' ' otherwise
__device__ __forceinline__ uint32_t put_char(uint8_t *s, uint32_t p, bool covered)
{
    if (covered) { s[p] = 0xe2; s[p + 1] = 0x96; s[p + 2] = 0x80; return p + 3; }
    s[p] = ' ';
    return p + 1;
}

// exclusive scan of one value per lane over the workgroup (wave prefix by __shfl_up, the wave totals through LDS); total: the sum
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
    for (int w = 0; w < kAnsiBlock / 64; w++) {
        const uint32_t s = wsum[w];
        before += w < wid ? s : 0u;
        total += s;
    }
    __syncthreads();                      // (wsum may be reused)
    return before + inc - v;
}

} // namespace ycge_ansi
