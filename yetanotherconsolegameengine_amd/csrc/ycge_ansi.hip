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
#include "ycge_ansi_cells.hip.h"

namespace {

using namespace ycge_ansi;          // the tile shape, cell_at, digits, the writers and the workgroup scan (shared with ycge_ansi_delta.hip)

constexpr int kAnsiCellMax = (5 + 10) + 20 + 3;                   // a row's cursor move (ten digits at most), the longest escape, '▀'
constexpr int kAnsiTileBytes = kAnsiTile * kAnsiCellMax;

// the bytes Render() writes for cell c behind a cell whose indices were (pfg, pbg) (256: none yet)
__device__ __forceinline__ uint32_t cell_bytes(const Cell &c, uint32_t pfg, uint32_t pbg)
{
    const uint32_t len = c.x == 0 ? 5u + digits(c.y + 1u) : 0u;      // ESC [ y+1 ; 1 H
    return len + sgr_bytes(c.fg, c.bg, pfg, pbg) + (c.covered ? 3u : 1u);
}

__device__ __forceinline__ uint32_t put_cell(uint8_t *s, uint32_t p, const Cell &c, uint32_t pfg, uint32_t pbg)
{
    if (c.x == 0) { p = put_ascii(s, p, "\x1b["); p = put_int(s, p, c.y + 1u); p = put_ascii(s, p, ";1H"); }
    return put_char(s, put_sgr(s, p, c.fg, c.bg, pfg, pbg), c.covered);
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
