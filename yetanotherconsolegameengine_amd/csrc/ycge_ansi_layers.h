// ycge_ansi_layers.h - what crosses from ycge_ansi.cpp into the kernel units for a layered ANSI stream (ycge_console_set_layers): the
// console's other framebuffers as the device holds them, and the planes of the composite.  Plain data, no HIP.
#pragma once
#include <cstdint>

namespace ycge_ansi {

constexpr int kMaxLayers = 16;                // YCGE_CONSOLE_MAX_LAYERS

struct LayerRect {
    int32_t x, y, w, h;                       // Framebuffer.ViewportX / ViewportY / Width / Height
    uint32_t first;                           // its cell (0, 0) in the layer arrays; cell (lx, ly) at first + ly * w + lx
};

// One layered stream.  The layers' cells lie one behind the other, `cells` in all: glyphs[k] the UTF-16 code unit of cell k, colours what
// k_encode_chexels writes for the cells as a cells x 1 framebuffer {top = foreground, bottom = background} in the call's colour form -
// pairs[2 k] / pairs[2 k + 1], or the RGBA words [k] / [cells + k].  The composite fills the console: a colour plane in the form of a
// cw x ch framebuffer's and a glyph plane of cw * ch code units.
struct LayersRun {
    int32_t n, raytrace_at;                   // rect[0..n) bottom first; raytrace_at of them lie below the raytrace framebuffer
    uint32_t cells;
    const uint8_t *colours;
    const uint16_t *glyphs;
    LayerRect rect[kMaxLayers];
    uint8_t *comp;                            // this call's composite, written by the compose kernel
    uint16_t *comp_glyph;
    const uint8_t *prev;                      // a delta: the composite the last stream handed out left on the terminal
    const uint16_t *prev_glyph;
    uint8_t *next;                            // a 24-bit delta: the colour plane that receives emitted ? cur : shown (the next glyph plane is comp_glyph)
};

} // namespace ycge_ansi
