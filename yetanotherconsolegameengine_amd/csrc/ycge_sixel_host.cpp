// ycge_sixel_host.cpp - the sixel streams in plain C++ from register planes: ycge_sixel_encode_host and ycge_sixel_encode_delta_host, the
// yardsticks of the kernels (ycge_sixel.hip) on a machine without a device and, under YCGE_SIXEL_HOST=1, the encoders of the stream calls on
// the planes read back (ycge_sixel.cpp).  No HIP, no context: see ycge_sixel_host.h.  Behind them the adaptive palette in the same way:
// ycge_sixel_palette_host and ycge_sixel_encode_palette_host, the yardsticks of ycge_sixel_palette.hip.
//
// The delta's bound.  A delta stream never exceeds ycge_sixel_stream_bound(W, H) = 3200 + bands * L * (W + 5) with L = min(216, 6 W):
//   - its header is the full one's without ESC[2J (4 bytes less) and with "0;1" in the introducer (3 bytes more): at most 24 + 6 + 26 + 3130
//     = 3186 bytes, the trailer 2 more, under the 3200 set aside;
//   - a changed band has at most min(216, 6 (hi - lo)) <= L lines, each at most #ddd, W characters (a run !<n>c is never longer than its n
//     columns) and one separator - its '$', or for the band's first line the one '-' in front of the band: the band's budget L (W + 5);
//   - an unchanged band in front of a changed one costs its '-', one byte, out of a budget of at least 6 * 6 = 36; bands behind the last
//     changed one cost nothing.
#include "ycge_sixel_host.h"

#include <cstring>
#include <vector>

#include "../../include/ycge.h"

namespace ycge_sixel_host {

namespace {

constexpr unsigned long long kOffsetLimit = 0xffffffffull;          // the kernels' offsets are 32-bit

// the line of register c over the band's rows: '#', the register, its sixels of columns lo .. hi - 1 (zero everywhere else) in runs, the
// empty tail omitted.  six: W bytes of scratch
void encode_line(const uint8_t *row0, int32_t W, int32_t rows, int32_t lo, int32_t hi, int c, std::vector<uint8_t> &six, std::string &s)
{
    s += '#'; s += std::to_string(c);
    int32_t width = 0;
    for (int32_t x = 0; x < hi; x++) {
        uint8_t b = 0;
        if (x >= lo)
            for (int32_t r = 0; r < rows; r++) b |= (uint8_t)((row0[(size_t)r * W + x] == c) << r);
        six[(size_t)x] = b;
        if (b) width = x + 1;
    }
    for (int32_t x = 0; x < width;) {
        int32_t n = 1;
        while (x + n < width && six[(size_t)(x + n)] == six[(size_t)x]) n++;
        const char ch = (char)(63 + six[(size_t)x]);
        if (n >= 4) { s += '!'; s += std::to_string(n); s += ch; }
        else s.append((size_t)n, ch);
        x += n;
    }
}

// the lines of the registers present in columns lo .. hi - 1 of a band, ascending, joined by '$'; the number of lines
uint32_t encode_band(const uint8_t *row0, int32_t W, int32_t rows, int32_t lo, int32_t hi, std::vector<uint8_t> &six, std::string &s, int registers = 216)
{
    bool present[256] = {};
    for (int32_t r = 0; r < rows; r++)
        for (int32_t x = lo; x < hi; x++) present[row0[(size_t)r * W + x]] = true;
    uint32_t lines = 0;
    for (int c = 0; c < registers; c++) {
        if (!present[c]) continue;
        if (lines) s += '$';
        lines++;
        encode_line(row0, W, rows, lo, hi, c, six, s);
    }
    return lines;
}

bool plane_ok(const uint8_t *p, size_t n, int registers = 216)
{
    for (size_t i = 0; i < n; i++)
        if (p[i] >= registers) return false;
    return true;
}

} // namespace

bool stream_bound(int64_t W, int64_t H, unsigned long long &bound)
{
    if (W <= 0 || H <= 0) return false;
    const unsigned __int128 bands = (unsigned __int128)((H + 5) / 6), colours = (unsigned __int128)(6 * W < 216 ? 6 * W : 216);
    const unsigned __int128 b = 3200 + bands * colours * (unsigned __int128)(W + 5);
    if (b > kOffsetLimit) return false;
    bound = (unsigned long long)b;
    return true;
}

std::string stream_prefix(int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool delta)
{
    std::string s;
    s.reserve(3200);
    if (clear && !delta) s += "\x1b[2J";
    s += "\x1b[" + std::to_string((int64_t)vy + 1) + ";" + std::to_string((int64_t)vx + 1) + "H";
    s += delta ? "\x1bP0;1q" : "\x1bPq";
    s += "\"1;1;" + std::to_string(W) + ";" + std::to_string(H);
    return s;
}

std::string stream_header(int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool delta)
{
    std::string s = stream_prefix(W, H, vx, vy, clear, delta);
    for (int i = 0; i < 216; i++)
        s += "#" + std::to_string(i) + ";2;" + std::to_string(20 * (i / 36)) + ";" + std::to_string(20 * (i / 6 % 6)) + ";" + std::to_string(20 * (i % 6));
    return s;
}

int encode(const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len)
{
    unsigned long long bound = 0;
    if (!index || !out || !out_len || vx < 0 || vy < 0 || !stream_bound(W, H, bound) || capacity < bound) return YCGE_ERR_INVALID_ARG;
    if (!plane_ok(index, (size_t)W * H)) return YCGE_ERR_INVALID_ARG;
    std::string s = stream_header(W, H, vx, vy, clear != 0);
    const int32_t bands = (H + 5) / 6;
    std::vector<uint8_t> six((size_t)W);
    for (int32_t k = 0; k < bands; k++) {
        (void)encode_band(index + (size_t)6 * k * W, W, H - 6 * k < 6 ? H - 6 * k : 6, 0, W, six, s);
        if (k + 1 < bands) s += '-';
    }
    s += "\x1b\\";
    if (s.size() > capacity) return YCGE_ERR_INTERNAL;
    std::memcpy(out, s.data(), s.size());
    *out_len = s.size();
    return YCGE_OK;
}

int encode_delta(const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity, size_t *out_len,
                 uint32_t *out_info)
{
    unsigned long long bound = 0;
    if (!prev || !index || !out || !out_len || vx < 0 || vy < 0 || !stream_bound(W, H, bound) || capacity < bound) return YCGE_ERR_INVALID_ARG;
    if (!plane_ok(prev, (size_t)W * H) || !plane_ok(index, (size_t)W * H)) return YCGE_ERR_INVALID_ARG;
    std::string s = stream_header(W, H, vx, vy, false, true);
    const int32_t bands = (H + 5) / 6;
    std::vector<uint8_t> six((size_t)W);
    uint32_t changed = 0, painted = 0, lines = 0;
    int32_t written = 0;                                             // bands whose '-' stands in the stream already
    for (int32_t k = 0; k < bands; k++) {
        const int32_t rows = H - 6 * k < 6 ? H - 6 * k : 6;
        const size_t at = (size_t)6 * k * W;
        int32_t lo = W, hi = 0;
        for (int32_t r = 0; r < rows; r++)
            for (int32_t x = 0; x < W; x++)
                if (prev[at + (size_t)r * W + x] != index[at + (size_t)r * W + x]) {
                    if (x < lo) lo = x;
                    if (x + 1 > hi) hi = x + 1;
                }
        if (hi == 0) continue;
        s.append((size_t)(k - written), '-');
        written = k;
        changed++;
        painted += (uint32_t)(hi - lo) * (uint32_t)rows;
        lines += encode_band(index + at, W, rows, lo, hi, six, s);
    }
    s += "\x1b\\";
    if (s.size() > capacity) return YCGE_ERR_INTERNAL;
    std::memcpy(out, s.data(), s.size());
    *out_len = s.size();
    if (out_info) { out_info[0] = 0; out_info[1] = changed; out_info[2] = painted; out_info[3] = lines; }
    return YCGE_OK;
}

// ---- the adaptive palette (the contract: include/ycge.h at ycge_render_frame_sixel_palette), pass for pass as k_pal_build of
// ycge_sixel_palette.hip runs it: the histogram, eight level-synchronous cut passes over the 32 768 bins, the registers

bool palette_stream_bound(int64_t W, int64_t H, unsigned long long &bound)
{
    if (W <= 0 || H <= 0) return false;
    const unsigned __int128 bands = (unsigned __int128)((H + 5) / 6), colours = (unsigned __int128)(6 * W < 256 ? 6 * W : 256);
    const unsigned __int128 b = 4700 + bands * colours * (unsigned __int128)(W + 5);
    if (b > kOffsetLimit) return false;
    bound = (unsigned long long)b;
    return true;
}

void palette_build(const uint8_t *rgba, size_t n, KeptPalette &K)
{
    std::vector<uint32_t> cnt(kPaletteBins, 0), sum(3 * (size_t)kPaletteBins, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t bin = palette_bin(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
        cnt[bin]++;
        for (int k = 0; k < 3; k++) sum[3 * (size_t)bin + k] += rgba[4 * i + k];
    }
    std::memset(&K, 0, sizeof K);
    const auto coord = [](uint32_t bin, int a) { return (int)(bin >> (10 - 5 * a) & 31u); };
    int boxes = 1;
    for (int pass = 0; pass < 8; pass++) {
        const int n0 = boxes;
        int lo[256][3], hi[256][3], axis[256], cut[256], label[256];
        for (int b = 0; b < n0; b++)
            for (int a = 0; a < 3; a++) { lo[b][a] = 32; hi[b][a] = -1; }
        for (uint32_t bin = 0; bin < kPaletteBins; bin++) {
            if (!cnt[bin]) continue;
            const int b = K.table[bin];
            for (int a = 0; a < 3; a++) {
                const int t = coord(bin, a);
                if (t < lo[b][a]) lo[b][a] = t;
                if (t > hi[b][a]) hi[b][a] = t;
            }
        }
        for (int b = 0; b < n0; b++) {
            axis[b] = -1;
            int best = 0;
            for (int a = 0; a < 3; a++)
                if (hi[b][a] - lo[b][a] > best) { best = hi[b][a] - lo[b][a]; axis[b] = a; }          // (ties: the first of r, g, b; an extent below 1: no split)
        }
        std::vector<uint64_t> marginal((size_t)n0 * 32, 0);
        for (uint32_t bin = 0; bin < kPaletteBins; bin++) {
            const int b = K.table[bin];
            if (cnt[bin] && axis[b] >= 0) marginal[(size_t)b * 32 + coord(bin, axis[b])] += cnt[bin];
        }
        for (int b = 0; b < n0; b++) {
            if (axis[b] < 0) continue;
            const int a = axis[b];
            uint64_t total = 0, acc = 0;
            for (int t = lo[b][a]; t <= hi[b][a]; t++) total += marginal[(size_t)b * 32 + t];
            cut[b] = hi[b][a] - 1;
            for (int t = lo[b][a]; t < hi[b][a]; t++) {
                acc += marginal[(size_t)b * 32 + t];
                if (2 * acc >= total) { cut[b] = t; break; }
            }
            label[b] = boxes++;
        }
        for (uint32_t bin = 0; bin < kPaletteBins; bin++) {
            const int b = K.table[bin];
            if (axis[b] >= 0 && coord(bin, axis[b]) > cut[b]) K.table[bin] = (uint8_t)label[b];
        }
    }
    K.count = boxes;
    std::vector<uint64_t> k(256, 0), S(3 * 256, 0);
    for (uint32_t bin = 0; bin < kPaletteBins; bin++) {
        const int b = K.table[bin];
        k[b] += cnt[bin];
        for (int ch = 0; ch < 3; ch++) S[3 * (size_t)b + ch] += sum[3 * (size_t)bin + ch];
    }
    for (int b = 0; b < boxes; b++) {
        for (int ch = 0; ch < 3; ch++) {
            const uint64_t m = k[b] ? (2 * S[3 * (size_t)b + ch] + k[b]) / (2 * k[b]) : 0;          // (n = 0 pixels: box 0 alone, empty)
            K.rgba[4 * b + ch] = (uint8_t)m;
            K.pct[3 * b + ch] = (uint8_t)((200 * m + 255) / 510);
        }
        K.rgba[4 * b + 3] = 255;
    }
}

void palette_map(const uint8_t *rgba, size_t n, const KeptPalette &K, uint8_t *index)
{
    for (size_t i = 0; i < n; i++) index[i] = K.table[palette_bin(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2])];
}

std::string palette_definitions(const uint8_t *pct, int32_t count)
{
    std::string s;
    s.reserve(4608);
    for (int i = 0; i < count; i++)
        s += "#" + std::to_string(i) + ";2;" + std::to_string(pct[3 * i]) + ";" + std::to_string(pct[3 * i + 1]) + ";" + std::to_string(pct[3 * i + 2]);
    return s;
}

int palette(const uint8_t *rgba, int32_t W, int32_t H, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count)
{
    if (!rgba || (!out_index && !out_palette && !out_pct && !out_count) || W <= 0 || H <= 0 || (int64_t)W * H > kPalettePixels) return YCGE_ERR_INVALID_ARG;
    std::vector<KeptPalette> K(1);
    palette_build(rgba, (size_t)W * H, K[0]);
    if (out_index) palette_map(rgba, (size_t)W * H, K[0], out_index);
    if (out_palette) std::memcpy(out_palette, K[0].rgba, sizeof K[0].rgba);
    if (out_pct) std::memcpy(out_pct, K[0].pct, sizeof K[0].pct);
    if (out_count) *out_count = K[0].count;
    return YCGE_OK;
}

int encode_palette(const uint8_t *index, const uint8_t *pct, int32_t count, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity,
                   size_t *out_len)
{
    unsigned long long bound = 0;
    if (!index || !pct || !out || !out_len || count < 1 || count > 256 || vx < 0 || vy < 0 || !palette_stream_bound(W, H, bound) || capacity < bound) return YCGE_ERR_INVALID_ARG;
    if (!plane_ok(index, (size_t)W * H, count)) return YCGE_ERR_INVALID_ARG;
    for (int i = 0; i < 3 * count; i++)
        if (pct[i] > 100) return YCGE_ERR_INVALID_ARG;
    std::string s = stream_prefix(W, H, vx, vy, clear != 0, false) + palette_definitions(pct, count);
    const int32_t bands = (H + 5) / 6;
    std::vector<uint8_t> six((size_t)W);
    for (int32_t k = 0; k < bands; k++) {
        (void)encode_band(index + (size_t)6 * k * W, W, H - 6 * k < 6 ? H - 6 * k : 6, 0, W, six, s, 256);
        if (k + 1 < bands) s += '-';
    }
    s += "\x1b\\";
    if (s.size() > capacity) return YCGE_ERR_INTERNAL;
    std::memcpy(out, s.data(), s.size());
    *out_len = s.size();
    return YCGE_OK;
}

} // namespace ycge_sixel_host
