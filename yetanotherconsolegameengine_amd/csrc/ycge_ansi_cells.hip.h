// ycge_ansi_cells.hip.h - the ANSI presenter's escape streams on the device, once, for both colour forms (host side: ycge_ansi.cpp; the
// contract: include/ycge.h at ycge_render_frame_ansi and ycge_render_frame_ansi_delta).  ycge_ansi.hip instantiates it with palette
// indices (256 colours), ycge_ansi_rgb.hip with sRGB8 triples (24-bit colour); everything here is inlined into the unit that includes it.
//
// The full stream.  ANSITerminalRenderer.Render() (ANSITerminalRenderer.cs:86-153) walks the console cells in raster order and writes,
// per row, a cursor move, and per cell an SGR escape for the colours that differ from the previous cell's, then the cell's character.
// Whichever branch of :118-139 runs, (currentFgIdx, currentBgIdx) equals the cell's own (fg, bg) after it: the bytes of cell i depend on
// cell i, on cell i - 1 in raster order (the cursor move resets no colour) and on "none yet" before the first cell.  So a cell's length
// is a local function and the stream is one exclusive prefix sum over the cells followed by a scatter - reduce-then-scan over tiles:
//   k_count<C>  per tile of kAnsiTile cells: its byte count
//   k_scan      one workgroup: the tiles' offsets (behind the clear-screen prefix), the trailer ESC[0m and the stream length
//   k_write<C>  per tile: the cells' lengths again, a workgroup scan, the bytes staged in LDS, then stored in order
// No workgroup waits on another's flag.  Offsets are 32-bit: the host refuses a console whose bound reaches 2^32.
//
// The delta stream.  With `prev` what the last stream handed out left on the terminal, `cur` this frame's plane and merge_gap = G in 0..8:
//   changed(x, y)  the cell is covered by the framebuffer and C::changed says its colours differ from prev's (256 colours: in either
//                  byte of the pair; 24-bit: the largest |cur - prev| over its six channels exceeds the tolerance)
//   emitted(x, y)  changed, or in the same row strictly between two changed cells a < x < b with b - a - 1 <= G, or the console's last
//                  cell (always: the cursor ends where the full stream leaves it, pending wrap included)
//   a run start    an emitted cell with x == 0 or (x - 1, y) not emitted: ESC[<y+1>;<x+1>H, then the both-differ escape unconditionally
//                  (Render()'s first branch against "none yet"); any other emitted cell writes the escape of Render()'s three branches
//                  against cur(x - 1, y) - its left neighbour is emitted, so that is what the terminal holds there; then the character;
//                  ESC[0m behind the last cell.  No clear prefix, no per-row move.
// Between a < x < b the nearest changed cells on either side decide: with dl = x - a and dr = b - x the cell is emitted when
// dl + dr <= G + 1.  So a cell's bytes depend on the cell, on its left neighbour and on the changed flags at most G + 1 cells either side
// in its own row, and the stream is again one exclusive prefix sum over the cells and a scatter:
//   k_delta_count<C>  per tile: its byte count and its changed / emitted / run-start counts
//   k_scan<true>      one workgroup: the tiles' offsets, the three counters' sums, the trailer ESC[0m and the stream length
//   k_delta_write<C>  per tile: the lengths again, a workgroup scan, the emitted cells' bytes staged in LDS, then stored in order; and
//                     C::store_next for every covered cell (24-bit: the next `prev`; 256 colours: nothing)
// A tile loads the changed flags of its cells and kHalo = 9 >= G + 1 cells either side into LDS once; the searches stop at the row's ends,
// so a window never crosses a row.
//
// The bound.  With E = C::kEscMax the longest escape (20 for two indices, 36 for two triples) a delta never exceeds the full stream's
// bound, 7 + 4 + sum over rows (5 + digits(y + 1)) + (E + 3) cw ch (ycge_ansi_stream_bound: E + 3 = 23; ycge_ansi_rgb_stream_bound: 39):
//   - An emitted cell that is no run start writes at most E + 3 bytes, its share of (E + 3) cw ch.
//   - A run start writes its move, 4 + digits(y + 1) + digits(x + 1), and at most E + 3 bytes, its share of (E + 3) cw ch.
//   - A run start at x == 0: its move is 5 + digits(y + 1), exactly the row's move in the bound, and a row has at most one such run.
//   - A run start at x >= 1: (x - 1, y) is not emitted and precedes no other run start, so its E + 3 bytes of the bound are unspent and
//     pay for the move: 4 + digits(y + 1) + digits(x + 1) <= 4 + 10 < E + 3 (14 < 23, 14 < 39), because the host refuses a console whose
//     bound reaches 2^32, so cw ch < 2^32 / (E + 3) and digits(ch) + digits(cw) <= digits(cw ch) + 1 <= 10.
//   - The trailer is the bound's 4.  So the delta is at most the bound less the 7 bytes of the clear prefix, which it never writes; the
//     2 x 1 console with both cells changed (and, in 24-bit colour, every channel three-digit) reaches exactly that.
//   - A layered stream (below) writes any UTF-16 code unit as a cell's character.  AppendCharUtf8 (:204-224) writes a code unit below
//     0x80 as 1 byte, below 0x800 as 2 and any other as 3 - a lone surrogate too, in its 3-byte form - so no character is longer than
//     the 3 bytes of '▀' that E + 3 counts, and every line above holds as it stands.
//
// Layers.  With the console's other framebuffers set (ycge_console_set_layers; LayersRun in ycge_ansi_layers.h) a stream is two steps:
//   k_compose<C>      one lane per console cell: GetChexelForPoint (:67-84) over the at most 17 sources, topmost first - a layer cell whose
//                     code unit is not ' ' wins, the raytrace framebuffer's chexels are '▀' and always win, nothing gives ' ' in the default
//                     colours - into a console-sized colour plane in C's own form and a uint16_t glyph plane beside it
//   the kernels above, instantiated with Layered<C>: the composite is a framebuffer that fills the console (every cell covered, viewport
//                     0, 0), the character comes from the glyph plane (PlaneGlyph) and is 1, 2 or 3 bytes; changed(x, y) also holds where the
//                     code unit differs from the previous composite's.  A differing glyph is always emitted, so the next glyph plane is this
//                     call's as it stands; the colour planes follow C::store_next as before.
// The unlayered instances (FixedGlyph) load no glyph and launch no compose pass; the LDS stages keep their sizes, a character being at most
// the 3 bytes they already count.
//
// LDS.  A cell is at most (5 + 10) + E + 3 bytes in the full stream and (4 + 10 + 10) + E + 3 in a delta, which sizes the stage of a
// tile's 1024 cells (4 a lane): 38 912 and 48 128 B for 256 colours; 55 296 and 64 512 B for 24-bit colour, two workgroups a CU of the
// 160 KB.  Fewer cells a lane would halve the stage but not the work: the kernels are bound by the stream's stores and the plane's loads,
// the lanes hold no state across cells that LDS capacity would let more waves hide, and a smaller tile doubles the tiles the
// one-workgroup scan walks.  Kept at 4.
//
// A colour policy C is a struct of static members, all inlined:
//   Plane           the plane's element type (uint8_t: {fg, bg} index pairs; uint32_t: RGBA words)
//   Delta           the delta kernels' arguments: DeltaArgs<Plane>, or a struct derived from it with the policy's own fields
//   kNone           "none yet": no colour equals it;  kEscMax: E above
//   offset(a, fx, fy)              where framebuffer cell (fx, fy) starts in a plane
//   load(p, a, fg, bg)             the colours of the covered cell at p;  load_default(a, fg, bg): those of any other cell
//   esc_bytes / put_esc(s, p, ..)  (fg, bg, pfg, pbg): the escape of Render()'s three branches behind (pfg, pbg), its length and its bytes
//   both_bytes(fg, bg)             the length of the both-differ escape, which a run start writes unconditionally
//   changed(d, o)                  changed, for the covered cell at offset o
//   store_next(d, o, emitted)      what k_delta_write leaves for the next call at offset o
//   Glyph                          FixedGlyph ('▀' where covered, ' ' elsewhere); Layered<C> has PlaneGlyph
//   store(p, a, fg, bg)            load's inverse, and layer_load(lc, cells, k, fg, bg): the colours of layer cell k (k_compose alone)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "ycge_ansi_layers.h"

namespace ycge_ansi {

constexpr int kAnsiBlock = 256;
constexpr int kAnsiPerLane = 4;                                   // consecutive cells per lane
constexpr int kAnsiTile = kAnsiBlock * kAnsiPerLane;
constexpr int kGapMax = 8;
constexpr int kHalo = kGapMax + 1;                                // changed flags either side of a tile
constexpr int kFlags = kAnsiTile + 2 * kHalo;
constexpr int kTileWords = 4;                                     // delta, per tile: bytes (then offset), changed, emitted, run starts

template <typename T>
struct StreamArgs {
    const T *plane;                       // what k_encode_chexels writes for the fbW x fbH framebuffer (C::offset, C::load)
    const T *palette;                     // that encoder on the 16 palette colours (C::load_default)
    int32_t fbW, fbH, cw, vx, vy, dfg, dbg;
    uint32_t n;                           // console cells, cw * ch
    const uint16_t *glyph;                // PlaneGlyph alone: the composite's code units, n of them (the plane is then cw x ch at 0, 0)
};

template <typename T>
struct DeltaArgs {
    StreamArgs<T> a;                      // a.plane: this frame's
    const T *prev;                        // what the last stream handed out left on the terminal, same shape
    int32_t gap;                          // merge_gap, 0..kGapMax
    const uint16_t *prev_glyph;           // PlaneGlyph alone: prev's code units
};

struct Cell {
    uint32_t x, y, fg, bg;
    uint32_t ch;                          // PlaneGlyph alone: the cell's UTF-16 code unit
    bool covered;                         // a framebuffer chexel ('▀'); otherwise the default cell (' ')
};

// The glyph policy.  FixedGlyph: the character is a compile-time function of `covered`, no plane is read.  PlaneGlyph: the composite of a
// layered console, whose every cell is covered and whose character is the glyph plane's code unit.
struct FixedGlyph { static constexpr bool kPlane = false; };
struct PlaneGlyph { static constexpr bool kPlane = true; };

// a colour policy over the composite of a layered console
template <class C>
struct Layered : C { using Glyph = PlaneGlyph; };

// A policy derived from FrameGlyphs too: the raytrace framebuffer's chexels carry a glyph of their own (the quadrant fit's, fbW * fbH code
// units, none of them ' ') where any other policy's are '▀'.  k_compose alone reads them; the streams of such a composite are Layered<C>'s.
struct FrameGlyphs {};
template <class C>
constexpr bool kFrameGlyphs = std::is_base_of<FrameGlyphs, C>::value;

// console cell (x, y) lies on the framebuffer; o: where its colours start in a plane
template <class C>
__device__ __forceinline__ bool covered_at(const StreamArgs<typename C::Plane> &a, uint32_t x, uint32_t y, size_t &o)
{
    if (C::Glyph::kPlane) { o = C::offset(a, x, y); return true; }
    const int64_t fx = (int64_t)x - a.vx, fy = (int64_t)y - a.vy;
    if (!(fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH)) return false;
    o = C::offset(a, (size_t)fx, (size_t)fy);
    return true;
}

// GetChexelForPoint (:67-84) with the raytrace framebuffer alone: its chexels are '▀', never ' ', so no layer below shows through
// (PlaneGlyph: the composite's cell, which k_compose made by that lookup over every source)
template <class C>
__device__ __forceinline__ Cell cell_at(const StreamArgs<typename C::Plane> &a, uint32_t i)
{
    Cell c;
    c.y = i / (uint32_t)a.cw;
    c.x = i - c.y * (uint32_t)a.cw;
    c.ch = 0;
    if (C::Glyph::kPlane) {
        c.covered = true;
        c.ch = a.glyph[i];
        C::load(a.plane + C::offset(a, c.x, c.y), a, c.fg, c.bg);
        return c;
    }
    const int64_t fx = (int64_t)c.x - a.vx, fy = (int64_t)c.y - a.vy;
    c.covered = fx >= 0 && fx < a.fbW && fy >= 0 && fy < a.fbH;
    if (c.covered) C::load(a.plane + C::offset(a, (size_t)fx, (size_t)fy), a, c.fg, c.bg);
    else C::load_default(a, c.fg, c.bg);
    return c;
}

// AppendInt (:181-202) on a non-negative value: its decimal digits, '0' for zero
__device__ __forceinline__ uint32_t digits(uint32_t v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
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

// the cell's character: '▀' U+2580 in UTF-8 when covered, ' ' otherwise
__device__ __forceinline__ uint32_t put_char(uint8_t *s, uint32_t p, bool covered)
{
    if (covered) { s[p] = 0xe2; s[p + 1] = 0x96; s[p + 2] = 0x80; return p + 3; }
    s[p] = ' ';
    return p + 1;
}

// the bytes of a cell's character.  PlaneGlyph: AppendCharUtf8 (:204-224) on the code unit - 1 byte below 0x80, 2 below 0x800, else 3
template <class G>
__device__ __forceinline__ uint32_t glyph_bytes(const Cell &c)
{
    if (G::kPlane) return 1u + (c.ch >= 0x80u) + (c.ch >= 0x800u);
    return c.covered ? 3u : 1u;
}

template <class G>
__device__ __forceinline__ uint32_t put_glyph(uint8_t *s, uint32_t p, const Cell &c)
{
    if (!G::kPlane) return put_char(s, p, c.covered);
    const uint32_t u = c.ch;
    if (u < 0x80u) { s[p] = (uint8_t)u; return p + 1; }
    if (u < 0x800u) { s[p] = (uint8_t)(0xc0u | u >> 6); s[p + 1] = (uint8_t)(0x80u | (u & 0x3fu)); return p + 2; }
    s[p] = (uint8_t)(0xe0u | u >> 12); s[p + 1] = (uint8_t)(0x80u | (u >> 6 & 0x3fu)); s[p + 2] = (uint8_t)(0x80u | (u & 0x3fu));
    return p + 3;
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

// ------------------------------------------------------------------------------------------------------------------ the full stream

// the bytes Render() writes for cell c behind a cell whose colours were (pfg, pbg) (kNone: none yet)
template <class C>
__device__ __forceinline__ uint32_t cell_bytes(const Cell &c, uint32_t pfg, uint32_t pbg)
{
    const uint32_t len = c.x == 0 ? 5u + digits(c.y + 1u) : 0u;      // ESC [ y+1 ; 1 H
    return len + C::esc_bytes(c.fg, c.bg, pfg, pbg) + glyph_bytes<typename C::Glyph>(c);
}

template <class C>
__device__ __forceinline__ uint32_t put_cell(uint8_t *s, uint32_t p, const Cell &c, uint32_t pfg, uint32_t pbg)
{
    if (c.x == 0) { p = put_ascii(s, p, "\x1b["); p = put_int(s, p, c.y + 1u); p = put_ascii(s, p, ";1H"); }
    return put_glyph<typename C::Glyph>(s, C::put_esc(s, p, c.fg, c.bg, pfg, pbg), c);
}

// the byte counts of this lane's kAnsiPerLane cells (a lane past the end counts 0)
template <class C>
__device__ __forceinline__ void lane_cells(const StreamArgs<typename C::Plane> &a, uint32_t first, Cell *cells, uint32_t *len)
{
    uint32_t pfg = C::kNone, pbg = C::kNone;
    if (first > 0 && first < a.n) { const Cell p = cell_at<C>(a, first - 1); pfg = p.fg; pbg = p.bg; }
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        len[k] = 0;
        if (first + k >= a.n) continue;
        cells[k] = cell_at<C>(a, first + k);
        len[k] = cell_bytes<C>(cells[k], pfg, pbg);
        pfg = cells[k].fg; pbg = cells[k].bg;
    }
}

// Kernels and launch helpers have internal linkage: each unit that includes this header registers its own instances with the runtime.
namespace {

template <class C>
__global__ __launch_bounds__(kAnsiBlock) void k_count(StreamArgs<typename C::Plane> a, uint32_t *__restrict__ tile_bytes)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane];
    lane_cells<C>(a, blockIdx.x * (uint32_t)kAnsiTile + threadIdx.x * (uint32_t)kAnsiPerLane, cells, len);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += len[k];
    (void)block_exclusive_scan(mine, wsum, total);
    if (threadIdx.x == 0) tile_bytes[blockIdx.x] = total;
}

// one workgroup, both forms: the tiles' byte counts -> offsets in place (full: one word a tile, behind the clear-screen prefix; DELTA:
// kTileWords a tile, and the three counters' sums); the trailer ESC[0m; res[0] the stream's length, DELTA: res[1..3] the counters
template <bool DELTA>
__global__ __launch_bounds__(kAnsiBlock) void k_scan(uint32_t *__restrict__ tiles, uint32_t n_tiles, int clear, uint8_t *__restrict__ out, uint32_t cap,
                                                      unsigned long long *__restrict__ res)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    constexpr uint32_t W = DELTA ? (uint32_t)kTileWords : 1u;
    uint32_t carry = clear ? 7u : 0u, counts[3] = {0, 0, 0};       // ESC [ 2 J ESC [ H (:100-103)
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
    if (threadIdx.x < 4 && carry + threadIdx.x < cap) out[carry + threadIdx.x] = (uint8_t)"\x1b[0m"[threadIdx.x];      // zeroSeq (:19, :149)
    if (threadIdx.x == 0) {
        res[0] = (unsigned long long)carry + 4ull;
        if (DELTA) { res[1] = sums[0]; res[2] = sums[1]; res[3] = sums[2]; }
    }
}

template <class C>
__global__ __launch_bounds__(kAnsiBlock) void k_write(StreamArgs<typename C::Plane> a, const uint32_t *__restrict__ tile_off, uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t stage[kAnsiTile * ((5 + 10) + C::kEscMax + 3)];      // a row's cursor move (ten digits at most), the longest escape, '▀'
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane];
    const uint32_t first = blockIdx.x * (uint32_t)kAnsiTile + threadIdx.x * (uint32_t)kAnsiPerLane;
    lane_cells<C>(a, first, cells, len);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += len[k];
    uint32_t p = block_exclusive_scan(mine, wsum, total);
    if (first < a.n) {
        uint32_t pfg = C::kNone, pbg = C::kNone;
        if (first > 0) { const Cell q = cell_at<C>(a, first - 1); pfg = q.fg; pbg = q.bg; }
#pragma unroll
        for (int k = 0; k < kAnsiPerLane; k++) {
            if (len[k] == 0) continue;
            p = put_cell<C>(stage, p, cells[k], pfg, pbg);
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

// ------------------------------------------------------------------------------------------------------------------ the delta stream

// changed(cell i), i < a.n
template <class C>
__device__ __forceinline__ bool changed_at(const typename C::Delta &d, uint32_t i)
{
    const uint32_t y = i / (uint32_t)d.a.cw, x = i - y * (uint32_t)d.a.cw;
    size_t o;
    if (!covered_at<C>(d.a, x, y, o)) return false;
    if (C::Glyph::kPlane && d.a.glyph[i] != d.prev_glyph[i]) return true;
    return C::changed(d, o);
}

// the changed flags of the tile at cell `tile0` and kHalo cells either side (0 outside the console) into flag[kFlags]
template <class C>
__device__ __forceinline__ void load_flags(const typename C::Delta &d, uint32_t tile0, uint8_t *flag)
{
    for (int j = threadIdx.x; j < kFlags; j += kAnsiBlock) {
        const int64_t i = (int64_t)tile0 - kHalo + j;
        flag[j] = i >= 0 && i < (int64_t)d.a.n ? (uint8_t)changed_at<C>(d, (uint32_t)i) : (uint8_t)0;
    }
    __syncthreads();
}

// emitted(cell i at column x), j its index in flag[] (kHalo - 1 <= j < kHalo + kAnsiTile): the searches stay inside the row and inside
// flag[] (j - gap >= 0, j + gap + 1 <= kFlags)
template <class D>
__device__ __forceinline__ bool emitted_at(const D &d, const uint8_t *flag, int j, uint32_t i, uint32_t x)
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
// start[k] (a run start) and pfg / pbg [k] (the colours of its left neighbour, read where it is no run start); counts {changed, emitted, run starts}
struct LaneCells {
    Cell cells[kAnsiPerLane];
    uint32_t len[kAnsiPerLane], pfg[kAnsiPerLane], pbg[kAnsiPerLane];
    bool start[kAnsiPerLane];
    uint32_t counts[3];
};

// STORE: also C::store_next for every covered cell of the lane
template <class C, bool STORE>
__device__ __forceinline__ void lane_delta(const typename C::Delta &d, const uint8_t *flag, uint32_t first, LaneCells &L)
{
    const StreamArgs<typename C::Plane> &a = d.a;
    L.counts[0] = L.counts[1] = L.counts[2] = 0;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) { L.len[k] = 0; L.start[k] = false; L.pfg[k] = L.pbg[k] = C::kNone; }
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
            size_t o;
            if (covered_at<C>(a, x, y, o)) C::store_next(d, o, em);
        }
        if (em) {
            const Cell c = cell_at<C>(a, i);
            L.cells[k] = c;
            L.start[k] = x == 0 || !left_emitted;
            uint32_t len;
            if (L.start[k]) {
                len = 4u + digits(y + 1u) + digits(x + 1u) + C::both_bytes(c.fg, c.bg);     // ESC [ y+1 ; x+1 H, the both-differ escape
            } else {
                const Cell p = left_loaded ? L.cells[k - 1 < 0 ? 0 : k - 1] : cell_at<C>(a, i - 1u);
                L.pfg[k] = p.fg; L.pbg[k] = p.bg;
                len = C::esc_bytes(c.fg, c.bg, p.fg, p.bg);
            }
            L.len[k] = len + glyph_bytes<typename C::Glyph>(c);
            L.counts[1]++;
            L.counts[2] += L.start[k];
        }
        left_emitted = em; left_loaded = em;
        if (++x == (uint32_t)a.cw) { x = 0; y++; }
    }
}

namespace {

template <class C>
__global__ __launch_bounds__(kAnsiBlock) void k_delta_count(typename C::Delta d, uint32_t *__restrict__ tiles)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t flag[kFlags];
    const uint32_t tile0 = blockIdx.x * (uint32_t)kAnsiTile;
    load_flags<C>(d, tile0, flag);
    LaneCells L;
    lane_delta<C, false>(d, flag, tile0 + threadIdx.x * (uint32_t)kAnsiPerLane, L);
    uint32_t mine = 0, total[kTileWords];
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += L.len[k];
    (void)block_exclusive_scan(mine, wsum, total[0]);
#pragma unroll
    for (int k = 0; k < 3; k++) (void)block_exclusive_scan(L.counts[k], wsum, total[k + 1]);
    if (threadIdx.x < kTileWords) tiles[blockIdx.x * (uint32_t)kTileWords + threadIdx.x] = total[threadIdx.x];
}

template <class C>
__global__ __launch_bounds__(kAnsiBlock) void k_delta_write(typename C::Delta d, const uint32_t *__restrict__ tiles, uint8_t *__restrict__ out, uint32_t cap)
{
    __shared__ uint32_t wsum[kAnsiBlock / 64];
    __shared__ uint8_t flag[kFlags];
    __shared__ uint8_t stage[kAnsiTile * ((4 + 10 + 10) + C::kEscMax + 3)];      // the cursor move, the longest escape, '▀'; only emitted cells are staged
    const uint32_t tile0 = blockIdx.x * (uint32_t)kAnsiTile;
    load_flags<C>(d, tile0, flag);
    LaneCells L;
    lane_delta<C, true>(d, flag, tile0 + threadIdx.x * (uint32_t)kAnsiPerLane, L);
    uint32_t mine = 0, total;
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) mine += L.len[k];
    uint32_t p = block_exclusive_scan(mine, wsum, total);
    if (total == 0) return;              // (uniform: a still tile stages and stores no byte)
#pragma unroll
    for (int k = 0; k < kAnsiPerLane; k++) {
        if (L.len[k] == 0) continue;
        const Cell &c = L.cells[k];
        if (L.start[k]) {
            p = put_ascii(stage, p, "\x1b["); p = put_int(stage, p, c.y + 1u); stage[p++] = ';'; p = put_int(stage, p, c.x + 1u); stage[p++] = 'H';
        }
        p = put_glyph<typename C::Glyph>(stage, C::put_esc(stage, p, c.fg, c.bg, L.pfg[k], L.pbg[k]), c);      // (a run start: against kNone, kNone - both colours)
    }
    __syncthreads();
    const uint32_t off = tiles[blockIdx.x * (uint32_t)kTileWords];
    for (uint32_t j = threadIdx.x; j < total; j += kAnsiBlock)
        if (off + j < cap) out[off + j] = stage[j];
}

// ------------------------------------------------------------------------------------------------------------------ the composite

template <typename T>
struct ComposeArgs {
    StreamArgs<T> a;                      // the raytrace framebuffer's plane, its geometry on the console, the default colours
    const T *layer_colours;               // LayersRun::colours
    const uint16_t *layer_glyphs;
    uint32_t layer_cells;
    int32_t n_layers, raytrace_at;
    T *out;                               // the composite's colour plane: a cw x ch framebuffer's
    uint16_t *out_glyph;                  // ... and its code units
    LayerRect rect[kMaxLayers];
};

// GetChexelForPoint (:67-84) for console cell i over every source.  Source s of 0..n_layers, bottom first: layer s below the raytrace
// framebuffer (s < raytrace_at), the raytrace framebuffer (s == raytrace_at), layer s - 1 above it.  Every index is checked against its
// rectangle before the load; the rectangles and `first` are the host's, within layer_cells.
template <class C>
__global__ __launch_bounds__(kAnsiBlock) void k_compose(ComposeArgs<typename C::Plane> g)
{
    const uint32_t i = blockIdx.x * (uint32_t)kAnsiBlock + threadIdx.x;
    if (i >= g.a.n) return;
    const uint32_t y = i / (uint32_t)g.a.cw, x = i - y * (uint32_t)g.a.cw;
    uint32_t fg = 0, bg = 0, ch = ' ';
    bool found = false;
    for (int s = g.n_layers; s >= 0 && !found; s--) {
        if (s == g.raytrace_at) {
            size_t o;
            if (covered_at<C>(g.a, x, y, o)) {
                C::load(g.a.plane + o, g.a, fg, bg);
                ch = kFrameGlyphs<C> ? (uint32_t)g.a.glyph[(size_t)((int64_t)y - g.a.vy) * (uint32_t)g.a.fbW + (size_t)((int64_t)x - g.a.vx)] : 0x2580u;
                found = true;
            }
            continue;
        }
        const LayerRect &r = g.rect[s < g.raytrace_at ? s : s - 1];
        const int64_t lx = (int64_t)x - r.x, ly = (int64_t)y - r.y;
        if (!(lx >= 0 && lx < r.w && ly >= 0 && ly < r.h)) continue;
        const uint32_t k = r.first + (uint32_t)ly * (uint32_t)r.w + (uint32_t)lx;
        const uint32_t u = g.layer_glyphs[k];
        if (u == (uint32_t)' ') continue;                            // (transparent whatever its colours)
        C::layer_load(g.layer_colours, g.layer_cells, k, fg, bg);
        ch = u; found = true;
    }
    if (!found) C::load_default(g.a, fg, bg);
    StreamArgs<typename C::Plane> full = g.a;                         // the composite as a framebuffer: cw wide
    full.fbW = g.a.cw;
    C::store(g.out + C::offset(full, x, y), full, fg, bg);
    g.out_glyph[i] = (uint16_t)ch;
}

// ------------------------------------------------------------------------------------------------------------------ the launch
//
// One StreamJob (ycge_ansi_layers.h), one check, one launcher.  launch<C, CC> runs the optional compose pass k_compose<CC>, then the
// stream kernels of C - over the framebuffer's plane - or of Layered<C> - over the composite: count, scan, write, or their delta forms.
// Three launches on `stream`, four with the compose pass.

inline uint32_t tiles_of(uint32_t cells) { return (cells + (uint32_t)kAnsiTile - 1u) / (uint32_t)kAnsiTile; }

// whether j is a job every kernel may see, its planes of T.  frame_glyphs: the compose policy reads the framebuffer's code units (the
// composite may then be of the framebuffer alone); stores_next: the policy's delta writes j.next under j.tol (24-bit colour)
template <typename T>
bool job_ok(const StreamJob &j, bool frame_glyphs, bool stores_next)
{
    const auto bad = [](const void *p) { return !p || (uintptr_t)p % alignof(T); };
    if (bad(j.plane) || bad(j.palette) || j.fbW <= 0 || j.fbH <= 0 || j.cw <= 0 || j.ch <= 0 || j.dfg < 0 || j.dfg > 15 || j.dbg < 0 || j.dbg > 15 ||
        (uint64_t)j.cw * (uint64_t)j.ch > 0xffffffffull || !j.tiles || !j.out || !j.res || j.cap > 0xffffffffull ||
        frame_glyphs != (j.frame_glyph != nullptr) || (frame_glyphs && !j.compose))
        return false;
    if (j.delta && (bad(j.prev) || (j.compose && !j.prev_glyph) || j.gap < 0 || j.gap > kGapMax)) return false;
    if (j.delta && stores_next &&
        (bad(j.next) || j.next == j.plane || j.next == j.prev || (j.compose && j.next == j.layers.comp) || j.tol < 0 || j.tol > 255))
        return false;
    if (!j.compose) return true;
    const LayersRun &L = j.layers;
    if (L.n < 0 || (L.n == 0 && !frame_glyphs) || L.n > kMaxLayers || L.raytrace_at < 0 || L.raytrace_at > L.n || (L.n > 0 && (!L.colours || !L.glyphs)) ||
        (uintptr_t)L.colours % alignof(T) || bad(L.comp) || !L.comp_glyph)
        return false;
    for (int k = 0; k < L.n; k++)
        if (L.rect[k].w <= 0 || L.rect[k].h <= 0 || (uint64_t)L.rect[k].first + (uint64_t)L.rect[k].w * (uint64_t)L.rect[k].h > (uint64_t)L.cells) return false;
    return true;
}

// the stream kernels of policy S over d.a
template <class S>
void launch_cells(const StreamJob &j, const typename S::Delta &d, hipStream_t stream)
{
    const uint32_t n_tiles = tiles_of(d.a.n), cap = (uint32_t)j.cap;
    const dim3 grid(n_tiles), block(kAnsiBlock);
    if (!j.delta) {
        hipLaunchKernelGGL(k_count<S>, grid, block, 0, stream, d.a, j.tiles);
        hipLaunchKernelGGL(k_scan<false>, dim3(1), block, 0, stream, j.tiles, n_tiles, j.clear, j.out, cap, j.res);
        hipLaunchKernelGGL(k_write<S>, grid, block, 0, stream, d.a, (const uint32_t *)j.tiles, j.out, cap);
    } else {
        hipLaunchKernelGGL(k_delta_count<S>, grid, block, 0, stream, d, j.tiles);
        hipLaunchKernelGGL(k_scan<true>, dim3(1), block, 0, stream, j.tiles, n_tiles, 0, j.out, cap, j.res);
        hipLaunchKernelGGL(k_delta_write<S>, grid, block, 0, stream, d, (const uint32_t *)j.tiles, j.out, cap);
    }
}

// d: the policy's own delta fields, set by the unit from the job (stores_next: it has them).  CC: the compose pass's policy, C or one
// derived from it with FrameGlyphs
template <class C, class CC = C>
int launch(const StreamJob &j, typename C::Delta d, bool stores_next, hipStream_t stream)
{
    using T = typename C::Plane;
    if (!job_ok<T>(j, kFrameGlyphs<CC>, stores_next)) return (int)hipErrorInvalidValue;
    StreamArgs<T> &a = d.a;
    a.plane = reinterpret_cast<const T *>(j.plane); a.palette = reinterpret_cast<const T *>(j.palette);
    a.fbW = j.fbW; a.fbH = j.fbH; a.cw = j.cw; a.vx = j.vx; a.vy = j.vy; a.dfg = j.dfg; a.dbg = j.dbg;
    a.n = (uint32_t)j.cw * (uint32_t)j.ch;
    a.glyph = nullptr;
    d.prev = reinterpret_cast<const T *>(j.prev); d.gap = j.gap; d.prev_glyph = nullptr;
    if (!j.compose) {
        launch_cells<C>(j, d, stream);
        return (int)hipGetLastError();
    }
    const LayersRun &L = j.layers;
    ComposeArgs<T> g;
    g.a = a;
    g.a.glyph = j.frame_glyph;
    for (int k = 0; k < kMaxLayers; k++) g.rect[k] = k < L.n ? L.rect[k] : LayerRect{0, 0, 0, 0, 0};
    g.layer_colours = reinterpret_cast<const T *>(L.colours); g.layer_glyphs = L.glyphs; g.layer_cells = L.cells;
    g.n_layers = L.n; g.raytrace_at = L.raytrace_at;
    g.out = reinterpret_cast<T *>(L.comp); g.out_glyph = L.comp_glyph;
    hipLaunchKernelGGL(k_compose<CC>, dim3((a.n + (uint32_t)kAnsiBlock - 1u) / (uint32_t)kAnsiBlock), dim3(kAnsiBlock), 0, stream, g);
    // the composite as the stream kernels' framebuffer: it fills the console
    a.plane = g.out; a.fbW = j.cw; a.fbH = j.ch; a.vx = 0; a.vy = 0; a.glyph = g.out_glyph;
    d.prev_glyph = j.prev_glyph;
    launch_cells<Layered<C>>(j, d, stream);
    return (int)hipGetLastError();
}

} // namespace

} // namespace ycge_ansi
