// ycge_ansi_rgb.hip - the 24-bit colour forms of the ANSI streams on the device: the full stream and the delta stream with a tolerance
// (host side: ycge_ansi.cpp; the contract: include/ycge.h at ycge_render_frame_ansi_rgb / ycge_render_frame_ansi_rgb_delta).
//
// The cells are those of ycge_ansi.hip with an sRGB8 triple where it has a palette index: a covered cell is ('▀', fg = RGB8(top),
// bg = RGB8(bottom)) read from the RGBA plane k_encode_chexels writes (fbW x 2 fbH words, row 2 cy the top half-cell, the fourth byte
// ignored), any other cell (' ', RGB8(palette[dfg]), RGB8(palette[dbg])) from the same encoder run on the 16 palette colours.  The
// escapes are Render()'s three branches (ANSITerminalRenderer.cs:118-139) with a triple for an index:
//   both differ  ESC[38;2;R;G;B;48;2;R;G;Bm   7 + 11 + 6 + 11 + 1 = 36 bytes at most
//   fg only      ESC[38;2;R;G;Bm              bg only  ESC[48;2;R;G;Bm      neither: nothing
// A cell's bytes are again a function of the cell and of its left neighbour in raster order, so both forms keep the scheme of ycge_ansi.hip
// and ycge_ansi_delta.hip - count per tile, one workgroup's scan, write through LDS - in three launches; no workgroup waits on another's flag.
//
// The delta form.  `shown` holds, per covered cell, the pair of triples the terminal displays (the RGBA plane's layout); with
// tolerance = T in 0..255 and merge_gap = G in 0..8:
//   changed(x, y)  the cell is covered and the largest |cur - shown| over its six channels exceeds T
//   emitted, run starts, cursor moves, the trailer: the rules of ycge_ansi_delta.hip, word for word (gap merge inside a row, the console's
//                  last cell always, a run start writes ESC[<y+1>;<x+1>H and the both-differ escape unconditionally, any other emitted
//                  cell the three branches against cur(x - 1, y) - its left neighbour is emitted, so that is what the terminal holds there)
// The write kernel stores the next `shown` - emitted ? cur : shown, for every covered cell - into a THIRD buffer: a tile reads the changed
// flags of up to 9 cells of its neighbours' tiles, so updating `shown` in place would race with them.  The host swaps the two on commit.
//
// The bound.  A delta never exceeds ycge_ansi_rgb_stream_bound(cw, ch) = 7 + 4 + sum over rows (5 + digits(y + 1)) + 39 cw ch:
//   - An emitted cell that is no run start writes at most 36 + 3 = 39 bytes, its share of 39 cw ch.
//   - A run start writes its move, 4 + digits(y + 1) + digits(x + 1), and at most 36 + 3 = 39 bytes, its share of 39 cw ch.
//   - A run start at x == 0: its move is 5 + digits(y + 1), exactly the row's move in the bound, and a row has at most one such run.
//   - A run start at x >= 1: (x - 1, y) is not emitted and precedes no other run start, so its 39 bytes of the bound are unspent and pay
//     for the move: 4 + digits(y + 1) + digits(x + 1) <= 4 + 10 < 39, because the host refuses a console whose bound reaches 2^32, so
//     cw ch < 2^32 / 39 and digits(ch) + digits(cw) <= digits(cw ch) + 1 <= 10.
//   - The trailer is the bound's 4.  So the delta is at most the bound less the 7 bytes of the clear prefix, which it never writes; the
//     2 x 1 console with both cells changed and every channel three-digit reaches exactly that.
//
// LDS.  The tile stays ycge_ansi_cells.hip.h's 1024 cells (4 a lane): the stage is 1024 x (15 + 36 + 3) = 55 296 B for the full form and
// 1024 x (24 + 36 + 3) = 64 512 B for the delta form, two workgroups a CU of the 160 KB.  Fewer cells a lane would halve the stage but not
// the work: the kernels are bound by the stream's stores and the plane's loads, the lanes hold no state across cells that LDS capacity
// would let more waves hide, and a smaller tile doubles the tiles the one-workgroup scan walks.  Kept at 4.
// Its own translation unit: the code objects of the 256-colour streams and of the frame kernels stay what they were.
#include "ycge_ansi_cells.hip.h"

namespace {

using namespace ycge_ansi;          // the tile shape, digits, put_int, put_ascii, put_char and the workgroup scan

constexpr uint32_t kNoColour = 0xffffffffu;                       // "none yet": no triple equals it
constexpr uint32_t kRgbMask = 0x00ffffffu;
constexpr int kRgbEscMax = 7 + 11 + 6 + 11 + 1;                   // 36
constexpr int kRgbCellMax = (5 + 10) + kRgbEscMax + 3;            // a row's cursor move (ten digits at most), the longest escape, '▀'
constexpr int kRgbTileBytes = kAnsiTile * kRgbCellMax;            // 55 296

constexpr int kGapMax = 8;
constexpr int kHalo = kGapMax + 1;                                // changed flags either side of a tile
constexpr int kFlags = kAnsiTile + 2 * kHalo;
constexpr int kRgbDeltaCellMax = (4 + 10 + 10) + kRgbEscMax + 3;  // the cursor move, the longest escape, '▀'
constexpr int kRgbDeltaTileBytes = kAnsiTile * kRgbDeltaCellMax;  // 64 512
constexpr int kTileWords = 4;                                     // delta, per tile: bytes (then offset), changed, emitted, run starts

struct RgbArgs {
    const uint32_t *rgba;                 // fbW x 2 fbH words R | G << 8 | B << 16 | (ignored) << 24, what k_encode_chexels writes
    const uint32_t *palette;              // that encoder on the palette as 8 chexels {palette[2 k], palette[2 k + 1]}: an 8 x 2 plane
    int32_t fbW, fbH, cw, vx, vy, dfg, dbg;
    uint32_t n;                           // console cells, cw * ch
};

// RGB8(palette[k]): chexel k / 2 of the 8 x 2 plane, top row for an even k
__device__ __forceinline__ uint32_t palette_rgb(const RgbArgs &a, int k) { return a.palette[(k & 1) * 8 + (k >> 1)] & kRgbMask; }

// the cell at raster index i; fg / bg: its triples as R | G << 8 | B << 16
__device__ __forceinline__ Cell rgb_cell_at(const RgbArgs &a, uint32_t i)
{
    Cell c;
    c.y = i / (uint32_t)a.cw;
    c.x = i - c.y * (uint32_t)a.cw;
    const int64_t fx = (int64_t)c.x - a.vx, fy = (int64_t)c.y - a.vy;
    c.covered = fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH;
    if (c.covered) {
        const uint32_t *p = a.rgba + (size_t)(2 * fy) * (uint32_t)a.fbW + (size_t)fx;
        c.fg = p[0] & kRgbMask; c.bg = p[a.fbW] & kRgbMask;
    } else {
        c.fg = palette_rgb(a, a.dfg); c.bg = palette_rgb(a, a.dbg);
    }
    return c;
}

// R;G;B as AppendInt writes the three: its length ...
__device__ __forceinline__ uint32_t triple_bytes(uint32_t c)
{
    const uint32_t r = c & 255u, g = c >> 8 & 255u, b = c >> 16 & 255u;
    return 5u + (r >= 10u) + (r >= 100u) + (g >= 10u) + (g >= 100u) + (b >= 10u) + (b >= 100u);
}

// ... and its bytes
__device__ __forceinline__ uint32_t put_triple(uint8_t *s, uint32_t p, uint32_t c)
{
    p = put_int(s, p, c & 255u); s[p++] = ';';
    p = put_int(s, p, c >> 8 & 255u); s[p++] = ';';
    return put_int(s, p, c >> 16 & 255u);
}

// the escape of Render()'s three branches for triples (fg, bg) behind (pfg, pbg) (kNoColour: none yet): its length
__device__ __forceinline__ uint32_t rgb_sgr_bytes(uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
{
    const bool f = fg != pfg, b = bg != pbg;
    if (f && b) return 14u + triple_bytes(fg) + triple_bytes(bg);  // ESC [ 3 8 ; 2 ; R;G;B ; 4 8 ; 2 ; R;G;B m
    if (f) return 8u + triple_bytes(fg);                          // ESC [ 3 8 ; 2 ; R;G;B m
    if (b) return 8u + triple_bytes(bg);                          // ESC [ 4 8 ; 2 ; R;G;B m
    return 0u;
}

__device__ __forceinline__ uint32_t put_rgb_sgr(uint8_t *s, uint32_t p, uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
{
    const bool f = fg != pfg, b = bg != pbg;
    if (f && b) { p = put_ascii(s, p, "\x1b[38;2;"); p = put_triple(s, p, fg); p = put_ascii(s, p, ";48;2;"); p = put_triple(s, p, bg); s[p++] = 'm'; }
    else if (f) { p = put_ascii(s, p, "\x1b[38;2;"); p = put_triple(s, p, fg); s[p++] = 'm'; }
    else if (b) { p = put_ascii(s, p, "\x1b[48;2;"); p = put_triple(s, p, bg); s[p++] = 'm'; }
    return p;
}

// ------------------------------------------------------------------------------------------------------------------ the full stream

__device__ __forceinline__ uint32_t cell_bytes(const Cell &c, uint32_t pfg, uint32_t pbg)
{
    const uint32_t len = c.x == 0 ? 5u + digits(c.y + 1u) : 0u;      // ESC [ y+1 ; 1 H
    return len + rgb_sgr_bytes(c.fg, c.bg, pfg, pbg) + (c.covered ? 3u : 1u);
}

__device__ __forceinline__ uint32_t put_cell(uint8_t *s, uint32_t p, const Cell &c, uint32_t pfg, uint32_t pbg)
{
    if (c.x == 0) { p = put_ascii(s, p, "\x1b["); p = put_int(s, p, c.y + 1u); p = put_ascii(s, p, ";1H"); }
    return put_char(s, put_rgb_sgr(s, p, c.fg, c.bg, pfg, pbg), c.covered);
}

// the byte counts of this lane's kAnsiPerLane cells (a lane past the end counts 0)
__device__ __forceinline__ void lane_cells(const RgbArgs &a, uint32_t first, Cell *cells, uint32_t *len)
{
    uint32_t pfg = kNoColour, pbg = kNoColour;
    if (first > 0 && first < a.n) { const Cell p = rgb_cell_at(a, first - 1); pfg = p.fg; pbg = p.bg; }
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        len[k] = 0;
        if (first + k >= a.n) continue;
        cells[k] = rgb_cell_at(a, first + k);
        len[k] = cell_bytes(cells[k], pfg, pbg);
        pfg = cells[k].fg; pbg = cells[k].bg;
    }
}

__global__ __launch_bounds__(kAnsiBlock) void k_rgb_count(RgbArgs a, uint32_t *__restrict__ tile_bytes)
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

// one workgroup, both forms: the tiles' byte counts -> offsets in place (full: one word a tile, behind the clear-screen prefix; DELTA:
// kTileWords a tile, and the three counters' sums); the trailer ESC[0m; res[0] the stream's length, DELTA: res[1..3] the counters
template <bool DELTA>
__global__ __launch_bounds__(kAnsiBlock) void k_rgb_scan(uint32_t *__restrict__ tiles, uint32_t n_tiles, int clear, uint8_t *__restrict__ out, uint32_t cap,
                                                          unsigned long long *__restrict__ res)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    constexpr uint32_t W = DELTA ? (uint32_t)kTileWords : 1u;
    uint32_t carry = clear ? 7u : 0u, counts[3] = {0, 0, 0};
    for (uint32_t base = 0; base < n_tiles; base += kAnsiBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t v = t < n_tiles ? tiles[t * W] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, total);
        if (t < n_tiles) {
            tiles[t * W] = carry + ex;
            if (DELTA) {
#pragma unroll
                for (int k = 0; k < 3; k++) counts[k] += tiles[t * W + 1 + k];
            }
        }
        carry += total;
    }
    uint32_t sums[3] = {0, 0, 0};
    if (DELTA) {
#pragma unroll
        for (int k = 0; k < 3; k++) (void)block_exclusive_scan(counts[k], wsum, sums[k]);
    }
    if (clear && threadIdx.x < 7 && threadIdx.x < cap) out[threadIdx.x] = (uint8_t)"\x1b[2J\x1b[H"[threadIdx.x];
    if (threadIdx.x < 4 && carry + threadIdx.x < cap) out[carry + threadIdx.x] = (uint8_t)"\x1b[0m"[threadIdx.x];
    if (threadIdx.x == 0) {
        res[0] = (unsigned long long)carry + 4ull;
        if (DELTA) { res[1] = sums[0]; res[2] = sums[1]; res[3] = sums[2]; }
    }
}

__global__ __launch_bounds__(kAnsiBlock) void k_rgb_write(RgbArgs a, const uint32_t *__restrict__ tile_off, uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t stage[kRgbTileBytes];
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane];
    const uint32_t first = blockIdx.x * (uint32_t)kAnsiTile + threadIdx.x * (uint32_t)kAnsiPerLane;
    lane_cells(a, first, cells, len);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += len[k];
    uint32_t p = block_exclusive_scan(mine, wsum, total);
    if (first < a.n) {
        uint32_t pfg = kNoColour, pbg = kNoColour;
        if (first > 0) { const Cell q = rgb_cell_at(a, first - 1); pfg = q.fg; pbg = q.bg; }
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

// ------------------------------------------------------------------------------------------------------------------ the delta stream

struct RgbDeltaArgs {
    RgbArgs a;                            // a.rgba: this frame's plane
    const uint32_t *shown;                // what the terminal displays, same shape
    uint32_t *next;                       // the next `shown`, same shape; written by k_rgb_delta_write for every covered cell
    int32_t gap, tol;                     // merge_gap 0..kGapMax, tolerance 0..255
};

// the largest |a - b| over the three channels of two words
__device__ __forceinline__ uint32_t max_channel_diff(uint32_t a, uint32_t b)
{
    const int d0 = abs((int)(a & 255u) - (int)(b & 255u));
    const int d1 = abs((int)(a >> 8 & 255u) - (int)(b >> 8 & 255u));
    const int d2 = abs((int)(a >> 16 & 255u) - (int)(b >> 16 & 255u));
    return (uint32_t)max(d0, max(d1, d2));
}

// changed(cell i), i < a.n
__device__ __forceinline__ bool changed_at(const RgbDeltaArgs &d, uint32_t i)
{
    const RgbArgs &a = d.a;
    const uint32_t y = i / (uint32_t)a.cw, x = i - y * (uint32_t)a.cw;
    const int64_t fx = (int64_t)x - a.vx, fy = (int64_t)y - a.vy;
    if (!(fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH)) return false;
    const size_t o = (size_t)(2 * fy) * (uint32_t)a.fbW + (size_t)fx;
    return max(max_channel_diff(a.rgba[o], d.shown[o]), max_channel_diff(a.rgba[o + a.fbW], d.shown[o + a.fbW])) > (uint32_t)d.tol;
}

// the changed flags of the tile at cell `tile0` and kHalo cells either side (0 outside the console) into flag[kFlags]
__device__ __forceinline__ void load_flags(const RgbDeltaArgs &d, uint32_t tile0, uint8_t *flag)
{
    for (int j = threadIdx.x; j < kFlags; j += kAnsiBlock) {
        const int64_t i = (int64_t)tile0 - kHalo + j;
        flag[j] = i >= 0 && i < (int64_t)d.a.n ? (uint8_t)changed_at(d, (uint32_t)i) : (uint8_t)0;
    }
    __syncthreads();
}

// emitted(cell i at column x), j its index in flag[] (kHalo - 1 <= j < kHalo + kAnsiTile): the searches stay inside the row and inside
// flag[] (j - gap >= 0, j + gap + 1 <= kFlags)
__device__ __forceinline__ bool emitted_at(const RgbDeltaArgs &d, const uint8_t *flag, int j, uint32_t i, uint32_t x)
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
// start[k] (a run start) and pfg / pbg [k] (the triples of its left neighbour, read where it is no run start); counts {changed, emitted, run starts}
struct LaneCells {
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane], pfg[kAnsiPerLane], pbg[kAnsiPerLane];
    bool start[kAnsiPerLane];
    uint32_t counts[3];
};

// STORE: also the next `shown` of every covered cell of the lane - emitted ? cur : shown, the fourth byte 255
template <bool STORE>
__device__ __forceinline__ void lane_delta(const RgbDeltaArgs &d, const uint8_t *flag, uint32_t first, LaneCells &L)
{
    const RgbArgs &a = d.a;
    L.counts[0] = L.counts[1] = L.counts[2] = 0;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) { L.len[k] = 0; L.start[k] = false; L.pfg[k] = L.pbg[k] = kNoColour; }
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
        if (STORE) {
            const int64_t fx = (int64_t)x - a.vx, fy = (int64_t)y - a.vy;
            if (fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH) {
                const size_t o = (size_t)(2 * fy) * (uint32_t)a.fbW + (size_t)fx;
                const uint32_t *src = em ? a.rgba : d.shown;
                d.next[o] = src[o] | 0xff000000u;
                d.next[o + a.fbW] = src[o + a.fbW] | 0xff000000u;
            }
        }
        if (em) {
            const Cell c = rgb_cell_at(a, i);
            L.cells[k] = c;
            L.start[k] = x == 0 || !left_emitted;
            uint32_t len;
            if (L.start[k]) {
                len = 4u + digits(y + 1u) + digits(x + 1u) + 14u + triple_bytes(c.fg) + triple_bytes(c.bg);     // ESC [ y+1 ; x+1 H, the both-differ escape
            } else {
                const Cell p = left_loaded ? L.cells[k - 1 < 0 ? 0 : k - 1] : rgb_cell_at(a, i - 1u);
                L.pfg[k] = p.fg; L.pbg[k] = p.bg;
                len = rgb_sgr_bytes(c.fg, c.bg, p.fg, p.bg);
            }
            L.len[k] = len + (c.covered ? 3u : 1u);
            L.counts[1]++;
            L.counts[2] += L.start[k];
        }
        left_emitted = em; left_loaded = em;
        if (++x == (uint32_t)a.cw) { x = 0; y++; }
    }
}

__global__ __launch_bounds__(kAnsiBlock) void k_rgb_delta_count(RgbDeltaArgs d, uint32_t *__restrict__ tiles)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t flag[kFlags];
    const uint32_t tile0 = blockIdx.x * (uint32_t)kAnsiTile;
    load_flags(d, tile0, flag);
    LaneCells L;
    lane_delta<false>(d, flag, tile0 + threadIdx.x * (uint32_t)kAnsiPerLane, L);
    uint32_t mine = 0, total[kTileWords];
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += L.len[k];
    (void)block_exclusive_scan(mine, wsum, total[0]);
#pragma unroll
    for (int k = 0; k < 3; k++) (void)block_exclusive_scan(L.counts[k], wsum, total[k + 1]);
    if (threadIdx.x < kTileWords) tiles[blockIdx.x * (uint32_t)kTileWords + threadIdx.x] = total[threadIdx.x];
}

__global__ __launch_bounds__(kAnsiBlock) void k_rgb_delta_write(RgbDeltaArgs d, const uint32_t *__restrict__ tiles, uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t flag[kFlags];
    __shared__ uint8_t stage[kRgbDeltaTileBytes];
    const uint32_t tile0 = blockIdx.x * (uint32_t)kAnsiTile;
    load_flags(d, tile0, flag);
    LaneCells L;
    lane_delta<true>(d, flag, tile0 + threadIdx.x * (uint32_t)kAnsiPerLane, L);       // (and the next `shown` of the tile's covered cells)
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += L.len[k];
    uint32_t p = block_exclusive_scan(mine, wsum, total);
    if (total == 0) return;               // (uniform: a still tile stages and stores no byte)
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        if (L.len[k] == 0) continue;
        const Cell &c = L.cells[k];
        if (L.start[k]) {
            p = put_ascii(stage, p, "\x1b["); p = put_int(stage, p, c.y + 1u); stage[p++] = ';'; p = put_int(stage, p, c.x + 1u); stage[p++] = 'H';
        }
        p = put_char(stage, put_rgb_sgr(stage, p, c.fg, c.bg, L.pfg[k], L.pbg[k]), c.covered);      // (a run start: against kNoColour - both triples)
    }
    __syncthreads();
    const uint32_t off = tiles[blockIdx.x * (uint32_t)kTileWords];
    for (uint32_t j = threadIdx.x; j < total; j += kAnsiBlock)
        if (off + j < cap) out[off + j] = stage[j];
}

bool fill_args(RgbArgs &a, const uint8_t *rgba, int fbW, int fbH, int cw, int ch, int vx, int vy, const uint8_t *palette, int dfg, int dbg)
{
    if (!rgba || !palette || fbW <= 0 || fbH <= 0 || cw <= 0 || ch <= 0 || dfg < 0 || dfg > 15 || dbg < 0 || dbg > 15 ||
        (uint64_t)cw * (uint64_t)ch > 0xffffffffull || ((uintptr_t)rgba & 3u) || ((uintptr_t)palette & 3u))
        return false;
    a.rgba = reinterpret_cast<const uint32_t *>(rgba); a.palette = reinterpret_cast<const uint32_t *>(palette);
    a.fbW = fbW; a.fbH = fbH; a.cw = cw; a.vx = vx; a.vy = vy; a.dfg = dfg; a.dbg = dbg;
    a.n = (uint32_t)cw * (uint32_t)ch;
    return true;
}

} // namespace

// the 24-bit stream of a cw x ch console over a fbW x 2 fbH RGBA plane at (vx, vy); palette: the 8 x 2 RGBA plane of the 16 palette colours,
// dfg / dbg their selection (0..15).  tiles: ycge_launch_ansi_tiles(cw * ch) words; out: cap bytes, at least the stream's bound (< 2^32);
// out_len: the stream's length.  Three launches on `stream`.
extern "C" int ycge_launch_ansi_rgb_stream(const uint8_t *rgba, int fbW, int fbH, int cw, int ch, int vx, int vy, const uint8_t *palette, int dfg, int dbg,
                                           int clear, uint32_t *tiles, uint8_t *out, unsigned long long cap, unsigned long long *out_len, hipStream_t stream)
{
    RgbArgs a;
    if (!fill_args(a, rgba, fbW, fbH, cw, ch, vx, vy, palette, dfg, dbg) || !tiles || !out || !out_len || cap > 0xffffffffull) return (int)hipErrorInvalidValue;
    const uint32_t n_tiles = (a.n + (uint32_t)kAnsiTile - 1u) / (uint32_t)kAnsiTile;
    hipLaunchKernelGGL(k_rgb_count, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, a, tiles);
    hipLaunchKernelGGL(k_rgb_scan<false>, dim3(1), dim3(kAnsiBlock), 0, stream, tiles, n_tiles, clear, out, (uint32_t)cap, out_len);
    hipLaunchKernelGGL(k_rgb_write, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, a, (const uint32_t *)tiles, out, (uint32_t)cap);
    return (int)hipGetLastError();
}

// the 24-bit delta stream of the plane `rgba` against `shown` for that geometry, merge_gap `gap` (0..8) and tolerance `tol` (0..255); next:
// a third plane of the same shape, distinct from both, that receives emitted ? cur : shown for every covered cell.  tiles: 4 *
// ycge_launch_ansi_tiles(cw * ch) words; res: 4 words {the stream's length, changed cells, emitted cells, run starts}.  Three launches.
extern "C" int ycge_launch_ansi_rgb_delta(const uint8_t *rgba, const uint8_t *shown, uint8_t *next, int fbW, int fbH, int cw, int ch, int vx, int vy,
                                          const uint8_t *palette, int dfg, int dbg, int gap, int tol, uint32_t *tiles, uint8_t *out, unsigned long long cap,
                                          unsigned long long *res, hipStream_t stream)
{
    RgbDeltaArgs d;
    if (!fill_args(d.a, rgba, fbW, fbH, cw, ch, vx, vy, palette, dfg, dbg) || !shown || !next || next == shown || next == rgba || ((uintptr_t)shown & 3u) ||
        ((uintptr_t)next & 3u) || !tiles || !out || !res || gap < 0 || gap > kGapMax || tol < 0 || tol > 255 || cap > 0xffffffffull)
        return (int)hipErrorInvalidValue;
    d.shown = reinterpret_cast<const uint32_t *>(shown); d.next = reinterpret_cast<uint32_t *>(next);
    d.gap = gap; d.tol = tol;
    const uint32_t n_tiles = (d.a.n + (uint32_t)kAnsiTile - 1u) / (uint32_t)kAnsiTile;
    hipLaunchKernelGGL(k_rgb_delta_count, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, d, tiles);
    hipLaunchKernelGGL(k_rgb_scan<true>, dim3(1), dim3(kAnsiBlock), 0, stream, tiles, n_tiles, 0, out, (uint32_t)cap, res);
    hipLaunchKernelGGL(k_rgb_delta_write, dim3(n_tiles), dim3(kAnsiBlock), 0, stream, d, (const uint32_t *)tiles, out, (uint32_t)cap);
    return (int)hipGetLastError();
}
