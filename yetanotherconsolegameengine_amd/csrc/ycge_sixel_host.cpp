// ycge_sixel_host.cpp - the sixel streams in plain C++ from register planes: ycge_sixel_encode_host and ycge_sixel_encode_delta_host, the
// yardsticks of the kernels (ycge_sixel.hip) on a machine without a device and, under YCGE_SIXEL_HOST=1, the encoders of the stream calls on
// the planes read back (ycge_sixel.cpp).  No HIP, no context: see ycge_sixel_host.h.
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
uint32_t encode_band(const uint8_t *row0, int32_t W, int32_t rows, int32_t lo, int32_t hi, std::vector<uint8_t> &six, std::string &s)
{
    bool present[216] = {};
    for (int32_t r = 0; r < rows; r++)
        for (int32_t x = lo; x < hi; x++) present[row0[(size_t)r * W + x]] = true;
    uint32_t lines = 0;
    for (int c = 0; c < 216; c++) {
        if (!present[c]) continue;
        if (lines) s += '$';
        lines++;
        encode_line(row0, W, rows, lo, hi, c, six, s);
    }
    return lines;
}

bool plane_ok(const uint8_t *p, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (p[i] >= 216) return false;
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

std::string stream_header(int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool delta)
{
    std::string s;
    s.reserve(3200);
    if (clear && !delta) s += "\x1b[2J";
    s += "\x1b[" + std::to_string((int64_t)vy + 1) + ";" + std::to_string((int64_t)vx + 1) + "H";
    s += delta ? "\x1bP0;1q" : "\x1bPq";
    s += "\"1;1;" + std::to_string(W) + ";" + std::to_string(H);
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

} // namespace ycge_sixel_host
