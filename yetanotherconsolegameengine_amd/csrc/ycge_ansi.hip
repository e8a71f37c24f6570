// ycge_ansi.hip - the 256-colour forms of the ANSI streams on the device: the full stream and the delta stream (host side: ycge_ansi.cpp;
// the contract: include/ycge.h at ycge_render_frame_ansi / ycge_render_frame_ansi_delta).
//
// The scheme, the delta rules and the bound are ycge_ansi_cells.hip.h's; this unit supplies the colours: a covered cell is ('▀',
// fg = ansi(top), bg = ansi(bottom)) read from the byte pairs k_encode_chexels writes, any other cell (' ', ansi(palette[dfg]),
// ansi(palette[dbg])) from the same encoder run on the 16 palette colours.  The escapes are Render()'s three branches
// (ANSITerminalRenderer.cs:118-139):
//   both differ  ESC[38;5;F;48;5;Bm   7 + 3 + 6 + 3 + 1 = 20 bytes at most
//   fg only      ESC[38;5;Fm          bg only  ESC[48;5;Bm      neither: nothing
// A delta's `prev` holds the pairs of the last stream handed out; a cell changed when its pair differs in either byte.
// Its own translation unit, as ycge_chexel.hip is: the code objects of the frame kernels stay what they were.
#include "ycge_ansi_cells.hip.h"

namespace {

using namespace ycge_ansi;

struct Indexed {
    using Plane = uint8_t;                // fbW x fbH {fg = ansi(top), bg = ansi(bottom)}; the palette: ansi(palette16[k]) at byte k
    using Args = StreamArgs<Plane>;
    using Delta = DeltaArgs<Plane>;
    using Glyph = FixedGlyph;
    static constexpr uint32_t kNone = 256u;
    static constexpr int kEscMax = 7 + 3 + 6 + 3 + 1;               // 20

    static __device__ __forceinline__ size_t offset(const Args &a, size_t fx, size_t fy) { return 2 * (fy * (uint32_t)a.fbW + fx); }
    static __device__ __forceinline__ void load(const Plane *p, const Args &, uint32_t &fg, uint32_t &bg) { fg = p[0]; bg = p[1]; }
    static __device__ __forceinline__ void load_default(const Args &a, uint32_t &fg, uint32_t &bg) { fg = a.palette[a.dfg]; bg = a.palette[a.dbg]; }
    static __device__ __forceinline__ void store(Plane *p, const Args &, uint32_t fg, uint32_t bg) { p[0] = (uint8_t)fg; p[1] = (uint8_t)bg; }
    // layer cell k of the pairs the encoder wrote for the layers' cells
    static __device__ __forceinline__ void layer_load(const Plane *lc, uint32_t, uint32_t k, uint32_t &fg, uint32_t &bg) { fg = lc[2 * (size_t)k]; bg = lc[2 * (size_t)k + 1]; }

    static __device__ __forceinline__ uint32_t both_bytes(uint32_t fg, uint32_t bg) { return 14u + digits(fg) + digits(bg); }

    static __device__ __forceinline__ uint32_t esc_bytes(uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
    {
        const bool f = fg != pfg, b = bg != pbg;
        if (f && b) return both_bytes(fg, bg);                    // ESC [ 3 8 ; 5 ; F ; 4 8 ; 5 ; B m
        if (f) return 8u + digits(fg);                            // ESC [ 3 8 ; 5 ; F m
        if (b) return 8u + digits(bg);                            // ESC [ 4 8 ; 5 ; B m
        return 0u;
    }

    static __device__ __forceinline__ uint32_t put_esc(uint8_t *s, uint32_t p, uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
    {
        const bool f = fg != pfg, b = bg != pbg;
        if (f && b) { p = put_ascii(s, p, "\x1b[38;5;"); p = put_int(s, p, fg); p = put_ascii(s, p, ";48;5;"); p = put_int(s, p, bg); s[p++] = 'm'; }
        else if (f) { p = put_ascii(s, p, "\x1b[38;5;"); p = put_int(s, p, fg); s[p++] = 'm'; }
        else if (b) { p = put_ascii(s, p, "\x1b[48;5;"); p = put_int(s, p, bg); s[p++] = 'm'; }
        return p;
    }

    static __device__ __forceinline__ bool changed(const Delta &d, size_t o) { return d.a.plane[o] != d.prev[o] || d.a.plane[o + 1] != d.prev[o + 1]; }
    static __device__ __forceinline__ void store_next(const Delta &, size_t, bool) {}      // (the frame's pairs are the next `prev` as they stand)
};

} // namespace

// the tiles of a console of `cells` cells: the length of the tile array a job is given
extern "C" uint32_t ycge_launch_ansi_tiles(uint32_t cells) { return tiles_of(cells); }

// The 256-colour stream of a job (ycge_ansi_layers.h): plane, prev and the composite are pairs, 2 bytes a cell; the palette the 16 default
// indices on the device.  Full or delta, with the compose pass or without; a job with frame glyphs is the other unit's and is refused.
extern "C" int ycge_launch_ansi_indexed(const StreamJob *j, hipStream_t stream)
{
    return j ? launch<Indexed>(*j, Indexed::Delta{}, false, stream) : (int)hipErrorInvalidValue;
}
