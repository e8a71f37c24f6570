// ycge_ansi_rgb.hip - the 24-bit colour forms of the ANSI streams on the device: the full stream and the delta stream with a tolerance
// (host side: ycge_ansi.cpp; the contract: include/ycge.h at ycge_render_frame_ansi_rgb / ycge_render_frame_ansi_rgb_delta).
//
// The scheme, the delta rules and the bound are ycge_ansi_cells.hip.h's; this unit supplies the colours, an sRGB8 triple where
// ycge_ansi.hip has a palette index: a covered cell is ('▀', fg = RGB8(top), bg = RGB8(bottom)) read from the RGBA plane k_encode_chexels
// writes (fbW x 2 fbH words, row 2 cy the top half-cell, the fourth byte ignored), any other cell (' ', RGB8(palette[dfg]),
// RGB8(palette[dbg])) from the same encoder run on the 16 palette colours.  The escapes are Render()'s three branches
// (ANSITerminalRenderer.cs:118-139) with a triple for an index:
//   both differ  ESC[38;2;R;G;B;48;2;R;G;Bm   7 + 11 + 6 + 11 + 1 = 36 bytes at most
//   fg only      ESC[38;2;R;G;Bm              bg only  ESC[48;2;R;G;Bm      neither: nothing
//
// The delta form.  `prev` is `shown`: per covered cell, the pair of triples the terminal displays (the RGBA plane's layout).  With
// tolerance = T in 0..255 a cell changed when the largest |cur - shown| over its six channels exceeds T.  The write kernel stores the next
// `shown` - emitted ? cur : shown, for every covered cell - into a THIRD buffer: a tile reads the changed flags of up to 9 cells of its
// neighbours' tiles, so updating `shown` in place would race with them.  The host swaps the two on commit.
// Its own translation unit: the code objects of the 256-colour streams and of the frame kernels stay what they were.
#include "ycge_ansi_cells.hip.h"

namespace {

using namespace ycge_ansi;

constexpr uint32_t kRgbMask = 0x00ffffffu;

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

// the largest |a - b| over the three channels of two words
__device__ __forceinline__ uint32_t max_channel_diff(uint32_t a, uint32_t b)
{
    const int d0 = abs((int)(a & 255u) - (int)(b & 255u));
    const int d1 = abs((int)(a >> 8 & 255u) - (int)(b >> 8 & 255u));
    const int d2 = abs((int)(a >> 16 & 255u) - (int)(b >> 16 & 255u));
    return (uint32_t)max(d0, max(d1, d2));
}

struct Rgb {
    using Plane = uint32_t;               // fbW x 2 fbH words R | G << 8 | B << 16 | (ignored) << 24; the palette: that encoder on 8 chexels
    using Args = StreamArgs<Plane>;       // {palette[2 k], palette[2 k + 1]}, an 8 x 2 plane
    struct Delta : DeltaArgs<Plane> {     // prev: `shown`
        Plane *next;                      // the next `shown`, same shape; written by k_delta_write for every covered cell
        int32_t tol;                      // tolerance 0..255
    };
    using Glyph = FixedGlyph;
    static constexpr uint32_t kNone = 0xffffffffu;                 // no triple equals it
    static constexpr int kEscMax = 7 + 11 + 6 + 11 + 1;            // 36

    static __device__ __forceinline__ size_t offset(const Args &a, size_t fx, size_t fy) { return 2 * fy * (uint32_t)a.fbW + fx; }
    static __device__ __forceinline__ void load(const Plane *p, const Args &a, uint32_t &fg, uint32_t &bg) { fg = p[0] & kRgbMask; bg = p[a.fbW] & kRgbMask; }
    // RGB8(palette[k]): chexel k / 2 of the 8 x 2 plane, top row for an even k
    static __device__ __forceinline__ uint32_t palette_rgb(const Args &a, int k) { return a.palette[(k & 1) * 8 + (k >> 1)] & kRgbMask; }
    static __device__ __forceinline__ void load_default(const Args &a, uint32_t &fg, uint32_t &bg) { fg = palette_rgb(a, a.dfg); bg = palette_rgb(a, a.dbg); }
    static __device__ __forceinline__ void store(Plane *p, const Args &a, uint32_t fg, uint32_t bg) { p[0] = fg | 0xff000000u; p[a.fbW] = bg | 0xff000000u; }
    // layer cell k of the plane the encoder wrote for the layers' cells as a cells x 1 framebuffer: the top row, then the bottom row
    static __device__ __forceinline__ void layer_load(const Plane *lc, uint32_t cells, uint32_t k, uint32_t &fg, uint32_t &bg)
    {
        fg = lc[k] & kRgbMask; bg = lc[(size_t)cells + k] & kRgbMask;
    }

    static __device__ __forceinline__ uint32_t both_bytes(uint32_t fg, uint32_t bg) { return 14u + triple_bytes(fg) + triple_bytes(bg); }

    static __device__ __forceinline__ uint32_t esc_bytes(uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
    {
        const bool f = fg != pfg, b = bg != pbg;
        if (f && b) return both_bytes(fg, bg);                        // ESC [ 3 8 ; 2 ; R;G;B ; 4 8 ; 2 ; R;G;B m
        if (f) return 8u + triple_bytes(fg);                          // ESC [ 3 8 ; 2 ; R;G;B m
        if (b) return 8u + triple_bytes(bg);                          // ESC [ 4 8 ; 2 ; R;G;B m
        return 0u;
    }

    static __device__ __forceinline__ uint32_t put_esc(uint8_t *s, uint32_t p, uint32_t fg, uint32_t bg, uint32_t pfg, uint32_t pbg)
    {
        const bool f = fg != pfg, b = bg != pbg;
        if (f && b) { p = put_ascii(s, p, "\x1b[38;2;"); p = put_triple(s, p, fg); p = put_ascii(s, p, ";48;2;"); p = put_triple(s, p, bg); s[p++] = 'm'; }
        else if (f) { p = put_ascii(s, p, "\x1b[38;2;"); p = put_triple(s, p, fg); s[p++] = 'm'; }
        else if (b) { p = put_ascii(s, p, "\x1b[48;2;"); p = put_triple(s, p, bg); s[p++] = 'm'; }
        return p;
    }

    static __device__ __forceinline__ bool changed(const Delta &d, size_t o)
    {
        const Plane *cur = d.a.plane;
        return max(max_channel_diff(cur[o], d.prev[o]), max_channel_diff(cur[o + d.a.fbW], d.prev[o + d.a.fbW])) > (uint32_t)d.tol;
    }

    // emitted ? cur : shown, the fourth byte 255
    static __device__ __forceinline__ void store_next(const Delta &d, size_t o, bool emitted)
    {
        const Plane *src = emitted ? d.a.plane : d.prev;
        d.next[o] = src[o] | 0xff000000u;
        d.next[o + d.a.fbW] = src[o + d.a.fbW] | 0xff000000u;
    }
};

// the quadrant-glyph streams' compose policy: Rgb, the raytrace framebuffer's chexels carrying the fitted glyph (k_fit_quadrants) for '▀'
struct RgbQuad : Rgb, FrameGlyphs {};

} // namespace

// The 24-bit stream of a job (ycge_ansi_layers.h): plane, prev, next and the composite are RGBA planes (w x 2 h words for w x h cells), the
// palette the 8 x 2 RGBA plane of the 16 palette colours.  Full or delta, with the compose pass or without; a delta's j->next receives
// emitted ? cur : shown for every covered cell under the tolerance j->tol.
// The quadrant-glyph forms (ycge_render_frame_ansi_quad / _quad_delta) are the jobs with frame_glyph, the fbW * fbH code units
// k_fit_quadrants wrote beside the plane, as the raytrace framebuffer's characters.  Every such stream is a composite's, so the job may
// hold no layer (n = 0: colours and glyphs unread).  One more instance, k_compose<RgbQuad>; the stream kernels are Layered<Rgb>'s.
extern "C" int ycge_launch_ansi_rgb(const StreamJob *j, hipStream_t stream)
{
    if (!j) return (int)hipErrorInvalidValue;
    Rgb::Delta d{};
    d.next = reinterpret_cast<uint32_t *>(j->next); d.tol = j->tol;
    return j->frame_glyph ? launch<Rgb, RgbQuad>(*j, d, true, stream) : launch<Rgb>(*j, d, true, stream);
}
