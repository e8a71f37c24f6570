// ycge_ansi.hip - the ANSI presenter's escape stream on the device (host side: ycge_ansi.cpp).
//
// ANSITerminalRenderer.Render() (ANSITerminalRenderer.cs:86-153) walks the console cells in raster order and writes, per row, a cursor
// move, and per cell an SGR escape for the indices that differ from the previous cell's, then the cell's character.  Whichever branch
// of :118-139 runs, (currentFgIdx, currentBgIdx) equals the cell's own (fg, bg) after it: the bytes of cell i depend on cell i, on cell
// i - 1 in raster order (the cursor move resets no colour) and on (-1, -1) before the first cell.  So a cell's length is a local
// function and the stream is one exclusive prefix sum over the cells followed by a scatter - reduce-then-scan over tiles:
//   k_ansi_count  per tile of kAnsiTile cells: its byte count
//   k_ansi_scan   one workgroup: the tiles' offsets (behind the clear-screen prefix), the trailer ESC[0m and the stream length
//   k_ansi_write  per tile: the cells' lengths again, a workgroup scan, the bytes staged in LDS, then stored in order
// No workgroup waits on another's flag.  Offsets are 32-bit: the host refuses a console whose bound reaches 2^32.
// Its own translation unit, as ycge_chexel.hip is: the code objects of the frame kernels stay what they were.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kAnsiBlock = 256;
constexpr int kAnsiPerLane = 4;                                   // consecutive cells per lane
constexpr int kAnsiTile = kAnsiBlock * kAnsiPerLane;
constexpr int kAnsiCellMax = (5 + 10) + 20 + 3;                   // a row's cursor move (ten digits at most), the longest escape, '▀'
constexpr int kAnsiTileBytes = kAnsiTile * kAnsiCellMax;

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

// the bytes Render() writes for cell c behind a cell whose indices were (pfg, pbg) (256: none yet)
__device__ __forceinline__ uint32_t cell_bytes(const Cell &c, uint32_t pfg, uint32_t pbg)
{
    uint32_t len = c.x == 0 ? 5u + digits(c.y + 1u) : 0u;            // ESC [ y+1 ; 1 H
    const bool f = c.fg != pfg, b = c.bg != pbg;
    if (f && b) len += 14u + digits(c.fg) + digits(c.bg);          // ESC [ 3 8 ; 5 ; F ; 4 8 ; 5 ; B m
    else if (f) len += 8u + digits(c.fg);                         // ESC [ 3 8 ; 5 ; F m
    else if (b) len += 8u + digits(c.bg);                         // ESC [ 4 8 ; 5 ; B m
    return len + (c.covered ? 3u : 1u);
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

__device__ __forceinline__ uint32_t put_cell(uint8_t *s, uint32_t p, const Cell &c, uint32_t pfg, uint32_t pbg)
{
    if (c.x == 0) { p = put_ascii(s, p, "\x1b["); p = put_int(s, p, c.y + 1u); p = put_ascii(s, p, ";1H"); }
    const bool f = c.fg != pfg, b = c.bg != pbg;
    if (f && b) { p = put_ascii(s, p, "\x1b[38;5;"); p = put_int(s, p, c.fg); p = put_ascii(s, p, ";48;5;"); p = put_int(s, p, c.bg); s[p++] = 'm'; }
    else if (f) { p = put_ascii(s, p, "\x1b[38;5;"); p = put_int(s, p, c.fg); s[p++] = 'm'; }
    else if (b) { p = put_ascii(s, p, "\x1b[48;5;"); p = put_int(s, p, c.bg); s[p++] = 'm'; }
    if (c.covered) { s[p] = 0xe2; s[p + 1] = 0x96; s[p + 2] = 0x80; return p + 3; }       // '▀' U+2580 in UTF-8
    s[p] = ' ';
    return p + 1;
}

// the byte counts of this lane's kAnsiPerLane cells (a lane past the end counts 0); prev: the indices of the cell before the first
__device__ __forceinline__ void lane_cells(const AnsiArgs &a, uint32_t first, Cell *cells, uint32_t *len)
{
    uint32_t pfg = 256u, pbg = 256u;
    if (first > 0 && first < a.n) { const Cell p = cell_at(a, first - 1); pfg = p.fg; pbg = p.bg; }
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        len[k] = 0;
        if (first + k >= a.n) continue;
        cells[k] = cell_at(a, first + k);
        len[k] = cell_bytes(cells[k], pfg, pbg);
        pfg = cells[k].fg; pbg = cells[k].bg;
    }
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

__global__ __launch_bounds__(kAnsiBlock) void k_ansi_count(AnsiArgs a, uint32_t *__restrict__ tile_bytes)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane];
    lane_cells(a, blockIdx.x * (uint32_t)kAnsiTile + threadIdx.x * (uint32_t)kAnsiPerLane, cells, len);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += len[k];
    (void)block_exclusive_scan(mine, wsum, total);
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = total;
}

// one workgroup: tile_bytes -> tile offsets in place; the clear-screen prefix, the trailer and the length
__global__ __launch_bounds__(kAnsiBlock) void k_ansi_scan(uint32_t *__restrict__ tiles, uint32_t n_tiles, int clear, uint8_t *__restrict__ out,
                                                           uint32_t cap, unsigned long long *__restrict__ out_len)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    uint32_t carry = clear ? 7u : 0u;                              // ESC [ 2 J ESC [ H (:100-103)
    for (uint32_t base = 0; base < n_tiles; base += kAnsiBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_tiles ? tiles[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, total);
        if (t < n_tiles) tiles[t] = carry + ex;
        carry += total;
    }
    if (clear && threadIdx.x < 7 && threadIdx.x < cap) out[threadIdx.x] = (uint8_t)"\x1b[2J\x1b[H"[threadIdx.x];
    if (threadIdx.x < 4 && carry + threadIdx.x < cap) out[carry + threadIdx.x] = (uint8_t)"\x1b[0m"[threadIdx.x];      // zeroSeq (:19, :149)
    if (threadIdx.x == 0) *out_len = (unsigned long long)carry + 4ull;
}

__global__ __launch_bounds__(kAnsiBlock) void k_ansi_write(AnsiArgs a, const uint32_t *__restrict__ tile_off, uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t stage[kAnsiTileBytes];
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane];
    const uint32_t first = blockIdx.x * (uint32_t)kAnsiTile + threadIdx.x * (uint32_t)kAnsiPerLane;
    lane_cells(a, first, cells, len);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += len[k];
    uint32_t p = block_exclusive_scan(mine, wsum, total);
    if (first < a.n) {
        uint32_t pfg = 256u, pbg = 256u;
        if (first > 0) { const Cell q = cell_at(a, first - 1); pfg = q.fg; pbg = q.bg; }
#pragma unroll
        for (int k = 0; k < kAnsiPerLane; k++) {
            if (len[k] == 0) continue;
            p = put_cell(stage, p, cells[k], pfg, pbg);
            pfg = cells[k].fg; pbg = cells[k].bg;
        }
    }
    __syncthreads();
    const uint32_t off = tile_off[blockIdx.x];
    // the tile's bytes in order: consecutive lanes, consecutive bytes (the bound check is the host's capacity, never reached)
    for (uint32_t j = threadIdx.x; j < total; j += kAnsiBlock)
        if (off + j < cap) out[off + j] = stage[j];
}

} // namespace

// the tiles of a console of `cells` cells: the length of the tile array that ycge_launch_ansi_stream is given
extern "C" uint32_t ycge_launch_ansi_tiles(uint32_t cells) { return (cells + (uint32_t)kAnsiTile - 1u) / (uint32_t)kAnsiTile; }

// the stream of a cw x ch console over a fbW x fbH framebuffer of ANSI pairs at (vx, vy); palette: the 16 default indices on the device,
// dfg / dbg their selection (0..15).  tiles: ycge_launch_ansi_tiles(cw * ch) words; out: cap bytes, at least the stream's bound (< 2^32);
// out_len: the stream's length.  Three launches on `stream`.
extern "C" int ycge_launch_ansi_stream(const uint8_t *pairs, int fbW, int fbH, int cw, int ch, int vx, int vy, const uint8_t *palette, int dfg, int dbg,
                                       int clear, uint32_t *tiles, uint8_t *out, unsigned long long cap, unsigned long long *out_len, hipStream_t stream)
{
    if (!pairs || !palette || !tiles || !out || !out_len || fbW <= 0 || fbH <= 0 || cw <= 0 || ch <= 0 || dfg < 0 || dfg > 15 || dbg < 0 || dbg > 15 ||
        (uint64_t)cw * (uint64_t)ch > 0xffffffffull || cap > 0xffffffffull)
        return (int)hipErrorInvalidValue;
    AnsiArgs a;
    a.pairs = pairs; a.palette = palette;
    a.fbW = fbW; a.fbH = fbH; a.cw = cw; a.vx = vx; a.vy = vy; a.dfg = dfg; a.dbg = dbg;
    a.n = (uint32_t)cw * (uint32_t)ch;
    const uint32_t n_tiles = ycge_launch_ansi_tiles(a.n);
    hipLaunchKernelGGL(k_ansi_count, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, a, tiles);
    hipLaunchKernelGGL(k_ansi_scan, dim3(1), dim3(kAnsiBlock), 0, stream, tiles, n_tiles, clear, out, (uint32_t)cap, out_len);
    hipLaunchKernelGGL(k_ansi_write, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, a, (const uint32_t *)tiles, out, (uint32_t)cap);
    return (int)hipGetLastError();
}
