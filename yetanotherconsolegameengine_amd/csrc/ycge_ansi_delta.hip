// ycge_ansi_delta.hip - the delta ANSI stream on the device: only the cells that changed since the last stream (host side:
// ycge_ansi.cpp; the contract: include/ycge.h at ycge_render_frame_ansi_delta).
//
// With `prev` the pairs of the last stream handed out and `cur` this frame's, and merge_gap = G in 0..8:
//   changed(x, y)  the cell is covered by the framebuffer and its pair differs from prev in either byte
//   emitted(x, y)  changed, or in the same row strictly between two changed cells a < x < b with b - a - 1 <= G, or the console's last
//                  cell (always: the cursor ends where the full stream leaves it, pending wrap included)
//   a run start    an emitted cell with x == 0 or (x - 1, y) not emitted: ESC[<y+1>;<x+1>H, then ESC[38;5;F;48;5;Bm unconditionally
//                  (Render()'s first branch against (-1, -1)); any other emitted cell writes the escape of Render()'s three branches
//                  against the pair of (x - 1, y); then the character; ESC[0m behind the last cell.  No clear prefix, no per-row move.
// Between a < x < b the nearest changed cells on either side decide: with dl = x - a and dr = b - x the cell is emitted when
// dl + dr <= G + 1.  So a cell's bytes depend on the cell, on its left neighbour and on the changed flags at most G + 1 cells either side
// in its own row, and the stream is again one exclusive prefix sum over the cells and a scatter, in the scheme of ycge_ansi.hip:
//   k_delta_count  per tile of kAnsiTile cells: its byte count and its changed / emitted / run-start counts
//   k_delta_scan   one workgroup: the tiles' offsets, the three counters' sums, the trailer ESC[0m and the stream length
//   k_delta_write  per tile: the lengths again, a workgroup scan, the emitted cells' bytes staged in LDS, then stored in order
// A tile loads the changed flags of its cells and kHalo = 9 >= G + 1 cells either side into LDS once; the searches stop at the row's ends,
// so a window never crosses a row.  No workgroup waits on another's flag.  Offsets are 32-bit, as in ycge_ansi.hip.
//
// The bound.  A delta never exceeds ycge_ansi_stream_bound(cw, ch) = 7 + 4 + sum over rows (5 + digits(y + 1)) + 23 cw ch:
//   - An emitted cell that is no run start writes at most 20 + 3 = 23 bytes, its share of 23 cw ch.
//   - A run start writes its move, 4 + digits(y + 1) + digits(x + 1), and at most 20 + 3 = 23 bytes, its share of 23 cw ch.
//   - A run start at x == 0: its move is 5 + digits(y + 1), exactly the row's move in the bound, and a row has at most one such run.
//   - A run start at x >= 1: (x - 1, y) is not emitted and precedes no other run start, so its 23 bytes of the bound are unspent and pay
//     for the move: 4 + digits(y + 1) + digits(x + 1) <= 4 + 10 < 23, because the host refuses a console whose bound reaches 2^32, so
//     cw ch < 2^32 / 23 and digits(ch) + digits(cw) <= digits(cw ch) + 1 <= 10.
//   - The trailer is the bound's 4.  So the delta is at most the bound less the 7 bytes of the clear prefix, which it never writes; the
//     2 x 1 console with both cells changed reaches exactly that.
// A cell is at most 4 + 10 + 10 + 20 + 3 = 47 bytes, which sizes the LDS stage; only emitted cells are staged.
// Its own translation unit: the code objects of the full stream's kernels stay what they were.
#include "ycge_ansi_cells.hip.h"

namespace {

using namespace ycge_ansi;

constexpr int kGapMax = 8;
constexpr int kHalo = kGapMax + 1;                                // changed flags either side of a tile
constexpr int kFlags = kAnsiTile + 2 * kHalo;
constexpr int kDeltaCellMax = (4 + 10 + 10) + 20 + 3;             // the cursor move, the longest escape, '▀'
constexpr int kDeltaTileBytes = kAnsiTile * kDeltaCellMax;        // 48 128
constexpr int kTileWords = 4;                                     // per tile: bytes (then offset), changed, emitted, run starts

struct DeltaArgs {
    AnsiArgs a;                           // a.pairs: this frame's
    const uint8_t *prev;                  // the pairs of the last stream handed out, same shape
    int32_t gap;                          // merge_gap, 0..kGapMax
};

// changed(cell i), i < a.n
__device__ __forceinline__ bool changed_at(const DeltaArgs &d, uint32_t i)
{
    const AnsiArgs &a = d.a;
    const uint32_t y = i / (uint32_t)a.cw, x = i - y * (uint32_t)a.cw;
    const int64_t fx = (int64_t)x - a.vx, fy = (int64_t)y - a.vy;
    if (!(fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH)) return false;
    const size_t o = 2 * ((size_t)fy * (uint32_t)a.fbW + (size_t)fx);
    return a.pairs[o] != d.prev[o] || a.pairs[o + 1] != d.prev[o + 1];
}

// the changed flags of the tile at cell `tile0` and kHalo cells either side (0 outside the console) into flag[kFlags]
__device__ __forceinline__ void load_flags(const DeltaArgs &d, uint32_t tile0, uint8_t *flag)
{
    for (int j = threadIdx.x; j < kFlags; j += kAnsiBlock) {
        const int64_t i = (int64_t)tile0 - kHalo + j;
        flag[j] = i >= 0 && i < (int64_t)d.a.n ? (uint8_t)changed_at(d, (uint32_t)i) : (uint8_t)0;
    }
    __syncthreads();
}

// emitted(cell i at column x), j its index in flag[] (kHalo - 1 <= j < kHalo + kAnsiTile): the searches stay inside the row and inside
// flag[] (j - gap >= 0, j + gap + 1 <= kFlags)
__device__ __forceinline__ bool emitted_at(const DeltaArgs &d, const uint8_t *flag, int j, uint32_t i, uint32_t x)
{
    if (flag[j] || i == d.a.n - 1u) return true;
    const int left = (int)min((uint32_t)d.gap, x), right = (int)min((uint32_t)d.gap, (uint32_t)d.a.cw - 1u - x);
    int dl = 0;
    for (int k = 1; k <= left; k++)
        if (flag[j - k]) { dl = k; break; }
    if (dl == 0) return false;
    for (int k = 1; k <= right && dl + k <= d.gap + 1; k++)
        if (flag[j + k]) return true;
    return false;
}

// one lane's kAnsiPerLane cells from `first`: len[k] the bytes of cell k (0: not emitted or past the end); for an emitted cell cells[k],
// start[k] (a run start) and pfg / pbg [k] (the pair of its left neighbour, read where it is no run start); counts {changed, emitted, run starts}
struct LaneCells {
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane], pfg[kAnsiPerLane], pbg[kAnsiPerLane];
    bool start[kAnsiPerLane];
    uint32_t counts[3];
};

__device__ __forceinline__ void lane_delta(const DeltaArgs &d, const uint8_t *flag, uint32_t first, LaneCells &L)
{
    const AnsiArgs &a = d.a;
    L.counts[0] = L.counts[1] = L.counts[2] = 0;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) { L.len[k] = 0; L.start[k] = false; L.pfg[k] = L.pbg[k] = 256u; }
    if (first >= a.n) return;
    const int j0 = kHalo + (int)(threadIdx.x * (uint32_t)kAnsiPerLane);
    uint32_t y = first / (uint32_t)a.cw, x = first - y * (uint32_t)a.cw;
    bool left_emitted = x > 0 && emitted_at(d, flag, j0 - 1, first - 1u, x - 1u), left_loaded = false;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        const uint32_t i = first + (uint32_t)k;
        if (i >= a.n) break;
        const bool em = emitted_at(d, flag, j0 + k, i, x);
        L.counts[0] += flag[j0 + k];
        if (em) {
            const Cell c = cell_at(a, i);
            L.cells[k] = c;
            L.start[k] = x == 0 || !left_emitted;
            uint32_t len;
            if (L.start[k]) {
                len = 4u + digits(y + 1u) + digits(x + 1u) + 14u + digits(c.fg) + digits(c.bg);     // ESC [ y+1 ; x+1 H, the two-index escape
            } else {
                const Cell p = left_loaded ? L.cells[k - 1 < 0 ? 0 : k - 1] : cell_at(a, i - 1u);
                L.pfg[k] = p.fg; L.pbg[k] = p.bg;
                len = sgr_bytes(c.fg, c.bg, p.fg, p.bg);
            }
            L.len[k] = len + (c.covered ? 3u : 1u);
            L.counts[1]++;
            L.counts[2] += L.start[k];
        }
        left_emitted = em; left_loaded = em;
        if (++x == (uint32_t)a.cw) { x = 0; y++; }
    }
}

__global__ __launch_bounds__(kAnsiBlock) void k_delta_count(DeltaArgs d, uint32_t *__restrict__ tiles)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t flag[kFlags];
    const uint32_t tile0 = blockIdx.x * (uint32_t)kAnsiTile;
    load_flags(d, tile0, flag);
    LaneCells L;
    lane_delta(d, flag, tile0 + threadIdx.x * (uint32_t)kAnsiPerLane, L);
    uint32_t mine = 0, total[kTileWords];
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += L.len[k];
    (void)block_exclusive_scan(mine, wsum, total[0]);
#pragma unroll
    for (int k = 0; k < 3; k++) (void)block_exclusive_scan(L.counts[k], wsum, total[k + 1]);
    if (threadIdx.x < kTileWords) tiles[blockIdx.x * (uint32_t)kTileWords + threadIdx.x] = total[threadIdx.x];
}

// one workgroup: the tiles' byte counts -> offsets in place; res = {stream length, changed, emitted, run starts}; the trailer
__global__ __launch_bounds__(kAnsiBlock) void k_delta_scan(uint32_t *__restrict__ tiles, uint32_t n_tiles, uint8_t *__restrict__ out, uint32_t cap,
                                                            unsigned long long *__restrict__ res)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    uint32_t carry = 0, counts[3] = {0, 0, 0};
    for (uint32_t base = 0; base < n_tiles; base += kAnsiBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_tiles ? tiles[t * kTileWords] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, total);
        if (t < n_tiles) {
            tiles[t * kTileWords] = carry + ex;
#pragma unroll
            for (int k = 0; k < 3; k++) counts[k] += tiles[t * kTileWords + 1 + k];
        }
        carry += total;
    }
    uint32_t sums[3];
#pragma unroll
    for (int k = 0; k < 3; k++) (void)block_exclusive_scan(counts[k], wsum, sums[k]);
    if (threadIdx.x < 4 && carry + threadIdx.x < cap) out[carry + threadIdx.x] = (uint8_t)"\x1b[0m"[threadIdx.x];
    if (threadIdx.x == 0) {
        res[0] = (unsigned long long)carry + 4ull;
        res[1] = sums[0]; res[2] = sums[1]; res[3] = sums[2];
    }
}

__global__ __launch_bounds__(kAnsiBlock) void k_delta_write(DeltaArgs d, const uint32_t *__restrict__ tiles, uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t flag[kFlags];
    __shared__ uint8_t stage[kDeltaTileBytes];
    const uint32_t tile0 = blockIdx.x * (uint32_t)kAnsiTile;
    load_flags(d, tile0, flag);
    LaneCells L;
    lane_delta(d, flag, tile0 + threadIdx.x * (uint32_t)kAnsiPerLane, L);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += L.len[k];
    uint32_t p = block_exclusive_scan(mine, wsum, total);
    if (total == 0) return;               // (uniform: a still tile stages and stores nothing)
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        if (L.len[k] == 0) continue;
        const Cell &c = L.cells[k];
        if (L.start[k]) {
            p = put_ascii(stage, p, "\x1b["); p = put_int(stage, p, c.y + 1u); stage[p++] = ';'; p = put_int(stage, p, c.x + 1u); stage[p++] = 'H';
        }
        p = put_char(stage, put_sgr(stage, p, c.fg, c.bg, L.pfg[k], L.pbg[k]), c.covered);      // (a run start: against 256, 256 - both indices)
    }
    __syncthreads();
    const uint32_t off = tiles[blockIdx.x * (uint32_t)kTileWords];
    for (uint32_t j = threadIdx.x; j < total; j += kAnsiBlock)
        if (off + j < cap) out[off + j] = stage[j];
}

} // namespace

// the delta stream of cur against prev (both fbW x fbH pairs) for the geometry of ycge_launch_ansi_stream and merge_gap `gap` (0..8).
// tiles: 4 * ycge_launch_ansi_tiles(cw * ch) words; out: cap bytes, at least the stream's bound (< 2^32); res: 4 words {the stream's
// length, changed cells, emitted cells, run starts}.  Three launches on `stream`.
extern "C" int ycge_launch_ansi_delta(const uint8_t *pairs, const uint8_t *prev, int fbW, int fbH, int cw, int ch, int vx, int vy, const uint8_t *palette,
                                      int dfg, int dbg, int gap, uint32_t *tiles, uint8_t *out, unsigned long long cap, unsigned long long *res,
                                      hipStream_t stream)
{
    if (!pairs || !prev || !palette || !tiles || !out || !res || fbW <= 0 || fbH <= 0 || cw <= 0 || ch <= 0 || dfg < 0 || dfg > 15 || dbg < 0 || dbg > 15 ||
        gap < 0 || gap > kGapMax || (uint64_t)cw * (uint64_t)ch > 0xffffffffull || cap > 0xffffffffull)
        return (int)hipErrorInvalidValue;
    DeltaArgs d;
    d.a.pairs = pairs; d.a.palette = palette;
    d.a.fbW = fbW; d.a.fbH = fbH; d.a.cw = cw; d.a.vx = vx; d.a.vy = vy; d.a.dfg = dfg; d.a.dbg = dbg;
    d.a.n = (uint32_t)cw * (uint32_t)ch;
    d.prev = prev; d.gap = gap;
    const uint32_t n_tiles = (d.a.n + (uint32_t)kAnsiTile - 1u) / (uint32_t)kAnsiTile;
    hipLaunchKernelGGL(k_delta_count, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, d, tiles);
    hipLaunchKernelGGL(k_delta_scan, dim3(1), dim3(kAnsiBlock), 0, stream, tiles, n_tiles, out, (uint32_t)cap, res);
    hipLaunchKernelGGL(k_delta_write, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, d, (const uint32_t *)tiles, out, (uint32_t)cap);
    return (int)hipGetLastError();
}
