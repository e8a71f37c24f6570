// ycge_sixel_host.h - the sixel streams in plain C++ (ycge_sixel_host.cpp): the bound, the header, the full stream and the delta stream of
// register planes.  No HIP and no context type: the file compiles on its own, and a stand-alone program can hold it to the contract under
// the host sanitizers (tests/sixel_host_main.cpp).  The contract: include/ycge.h at ycge_render_frame_sixel and ycge_render_frame_sixel_delta.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace ycge_sixel_host {

// 3200 + ceil(H / 6) * min(216, 6 W) * (W + 5); false where W or H is not positive or the bound does not fit 32 bits (the kernels' offsets)
bool stream_bound(int64_t W, int64_t H, unsigned long long &bound);

// parts 1 to 5 of the full stream; delta: the delta stream's parts 1 to 4 - no ESC[2J, and the introducer ESC P 0;1 q (P2 = 1: a zero bit
// leaves its pixel as it is)
std::string stream_header(int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool delta = false);

// parts 1 to 4 alone: everything in front of the register definitions
std::string stream_prefix(int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool delta = false);

// ycge_sixel_encode_host and ycge_sixel_encode_delta_host: status codes of include/ycge.h
int encode(const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len);
int encode_delta(const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity, size_t *out_len,
                 uint32_t *out_info);

// ---- the adaptive palette (the contract: include/ycge.h at ycge_render_frame_sixel_palette)
constexpr uint32_t kPaletteBins = 32768;
constexpr int64_t kPalettePixels = (int64_t)1 << 24;          // W * H above it is refused: a bin's byte sums are 32-bit
inline uint32_t palette_bin(uint8_t r, uint8_t g, uint8_t b) { return (uint32_t)(r >> 3) << 10 | (uint32_t)(g >> 3) << 5 | (uint32_t)(b >> 3); }
// what a context keeps of a palette: the box of every bin, the registers' bytes m (RGBA8, alpha 255, unused entries zero), their sixel
// percentages (unused entries zero) and how many registers there are
struct KeptPalette { uint8_t table[kPaletteBins]; uint8_t rgba[1024]; uint8_t pct[768]; int32_t count; };
// the palette block a context keeps on the device (ycge_sixel_palette.hip writes it), byte offsets: the stream's length (uint64: the
// encoder's scan), n and the definitions' length (uint32), the bytes, the percentages, the definitions, the table.  Its head - everything
// in front of the definitions - is what a call copies back
constexpr uint32_t kPalLength = 0, kPalCount = 8, kPalDefsBytes = 12, kPalRgba = 16, kPalPct = 1040, kPalDefs = 1808, kPalTable = 6416;
constexpr uint32_t kPalHeadBytes = kPalDefs, kPalBlockBytes = kPalTable + kPaletteBins;

// 4700 + ceil(H / 6) * min(256, 6 W) * (W + 5); refusals as stream_bound's
bool palette_stream_bound(int64_t W, int64_t H, unsigned long long &bound);
// the palette of n RGBA8 pixels; the register plane of n pixels through a palette (total: every bin has a box)
void palette_build(const uint8_t *rgba, size_t n, KeptPalette &K);
void palette_map(const uint8_t *rgba, size_t n, const KeptPalette &K, uint8_t *index);
// #i;2;pr;pg;pb for registers 0 .. count - 1
std::string palette_definitions(const uint8_t *pct, int32_t count);
// ycge_sixel_palette_host and ycge_sixel_encode_palette_host: status codes of include/ycge.h
int palette(const uint8_t *rgba, int32_t W, int32_t H, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count);
int encode_palette(const uint8_t *index, const uint8_t *pct, int32_t count, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity,
                   size_t *out_len);

} // namespace ycge_sixel_host
