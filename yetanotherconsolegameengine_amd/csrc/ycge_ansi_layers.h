// ycge_ansi_layers.h - what crosses from ycge_ansi.cpp into the kernel units for an ANSI stream: the one job descriptor of a stream call
// and, for a layered one (ycge_console_set_layers), the console's other framebuffers as the device holds them with the planes of the
// composite.  Plain data, no HIP.
#pragma once
#include <cstdint>

namespace ycge_ansi {

constexpr int kMaxLayers = 16;                // YCGE_CONSOLE_MAX_LAYERS

struct LayerRect {
    int32_t x, y, w, h;                       // Framebuffer.ViewportX / ViewportY / Width / Height
    uint32_t first;                           // its cell (0, 0) in the layer arrays; cell (lx, ly) at first + ly * w + lx
};

// The compose pass of a stream.  The layers' cells lie one behind the other, `cells` in all: glyphs[k] the UTF-16 code unit of cell k,
// colours what k_encode_chexels writes for the cells as a cells x 1 framebuffer {top = foreground, bottom = background} in the call's
// colour form - pairs[2 k] / pairs[2 k + 1], or the RGBA words [k] / [cells + k].  The composite fills the console: a colour plane in the
// form of a cw x ch framebuffer's and a glyph plane of cw * ch code units.
struct LayersRun {
    int32_t n, raytrace_at;                   // rect[0..n) bottom first; raytrace_at of them lie below the raytrace framebuffer
    uint32_t cells;
    const uint8_t *colours;
    const uint16_t *glyphs;
    LayerRect rect[kMaxLayers];
    uint8_t *comp;                            // this call's composite, written by the compose kernel
    uint16_t *comp_glyph;
};

// One stream call, whole: what ycge_launch_ansi_indexed / ycge_launch_ansi_rgb are given.  The stream kernels walk `plane`, or with
// `compose` the composite that the compose pass makes of it and the layers first; prev / prev_glyph / next have that plane's shape.
struct StreamJob {
    const uint8_t *plane;                     // the fbW x fbH framebuffer's colour plane in the unit's form (the pairs; the RGBA plane)
    const uint16_t *frame_glyph;              // the quadrant family: its fbW * fbH fitted code units (then `compose` is set); else NULL
    int32_t fbW, fbH, cw, ch, vx, vy;
    const uint8_t *palette;                   // the encoder's output for the 16 palette colours; dfg / dbg their selection (0..15)
    int32_t dfg, dbg;
    bool delta;                               // the delta kernels, against prev; otherwise the full stream's
    int32_t clear;                            // full: the clear-screen prefix
    int32_t gap, tol;                         // delta: merge_gap (0..8); 24-bit: the tolerance (0..255)
    const uint8_t *prev;                      // delta: what the last stream handed out left on the terminal
    const uint16_t *prev_glyph;               // ... and with `compose` its code units
    uint8_t *next;                            // 24-bit delta: the plane that receives emitted ? cur : shown, distinct from every other
    bool compose;                             // the compose pass in front; n == 0 (the framebuffer alone) with frame_glyph only
    LayersRun layers;
    uint32_t *tiles;                          // ycge_launch_ansi_tiles(cw * ch) words, a delta four times as many
    uint8_t *out;                             // cap bytes, at least the stream's bound (< 2^32)
    unsigned long long cap;
    unsigned long long *res;                  // {the stream's length; delta: changed cells, emitted cells, run starts}
};

} // namespace ycge_ansi
