// ycge_obj.h - MeshLoader.FromObj's reading rules (RayTracing/MeshLoader.cs:23-55, 99-105), written once for the host parser
// (ycge_obj_parse_host, below) and for the kernels of ycge_obj.hip.  Plain C++: no runtime, no context (a stand-alone program can include it).
//
// THE CONTRACT (tests/obj_restatement.py states it again in Python, sharing nothing with this file):
//   lines    StreamReader.ReadLine: a line ends at \n, \r\n or a lone \r; the last line needs no terminator (a terminator at the very end
//            opens no further line).  A UTF-8 byte-order mark at offset 0 is skipped.  Lines are numbered from 1, empty ones included.
//            A line that is empty or whose FIRST byte is '#' is skipped (" # x" is not: its first token is neither v nor f).
//   tokens   Split((char[])null, RemoveEmptyEntries): char.IsWhiteSpace.  In ASCII, inside a line: space, \t, \v, \f.  0x1C..0x1F are NOT
//            separators (they are for Python's str.split).
//   v        first token exactly "v", at least 4 tokens: tokens 1..3 are floats, the rest are never looked at.  Fewer tokens: no position.
//   f        first token exactly "f", at least 4 tokens: EVERY token is cut at its first '/', the part in front is an integer i (empty: index
//            0): i > 0 names i - 1, else count + i with count = positions read so far AT THIS LINE.  Fan (v0, v[k-1], v[k]), tokens - 3
//            triangles.  An index may name a position a later line defines: 0 <= index < final count is checked after the whole file.
//   floats   [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?, the whole token; the value is the decimal CORRECTLY ROUNDED to
//            binary32 (nearest, ties to even; -0 stays -0; overflow +-inf, underflow subnormal or zero) - what .NET's float.Parse gives,
//            not decimal -> binary64 -> binary32.  .NET's extras (thousands separators, Infinity, NaN, blanks) are refused, not imitated.
//   integers [+-]? digits, within int32.
//   refusals YCGE_ERR_INVALID_ARG unless said otherwise, in this order: the FIRST line in file order that holds a malformed float or
//            integer token or - YCGE_ERR_UNSUPPORTED - a byte >= 0x80 outside a comment (such a line would need .NET's Unicode
//            separators; the byte decides for its whole line); more than 2^28 triangles; no position or no triangle
//            (InvalidDataException); an index out of range, named by the lowest triangle in file order (counted from 0).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define YCGE_OBJ_HD __host__ __device__ inline
#else
#define YCGE_OBJ_HD inline
#endif

namespace ycge_obj {

constexpr uint32_t kLineCap = 1024;                  // bytes of a line (without its terminator) the kernels walk; a longer one that is no comment declines the file
constexpr int64_t kMaxTriangles = (int64_t)1 << 28;
// the low byte of an error key (line << 8 | code): the lowest key is the file's verdict
enum { BAD_FLOAT = 1, BAD_INT = 2, NON_ASCII = 3 };
// why the device did not parse (ycge_debug_obj_stats, out6[2]); the kernels set the first two
enum { DECLINE_FLOAT_DOMAIN = 1, DECLINE_LINE_CAP = 2, DECLINE_ENV_HOST = 4, DECLINE_BELOW_MIN = 8 };

YCGE_OBJ_HD bool is_sep(uint8_t b) { return b == ' ' || b == '\t' || b == 0x0b || b == 0x0c; }

// the next token of [p, e): [a, b); false at the end of the line
YCGE_OBJ_HD bool next_token(const uint8_t *t, uint32_t &p, uint32_t e, uint32_t &a, uint32_t &b)
{
    while (p < e && is_sep(t[p])) p++;
    if (p >= e) return false;
    a = p;
    while (p < e && !is_sep(t[p])) p++;
    b = p;
    return true;
}

// one walk over the line [s, e): 0 nothing, 1 a `v` line that adds a position, 2 an `f` line that adds `tris` triangles; non_ascii: a byte >= 0x80
// on a line that is no comment (the line then adds nothing)
YCGE_OBJ_HD int classify_line(const uint8_t *t, uint32_t s, uint32_t e, uint32_t &tris, bool &non_ascii)
{
    tris = 0; non_ascii = false;
    if (s >= e || t[s] == '#') return 0;
    uint32_t tokens = 0, first_len = 0;
    uint8_t first = 0, hi = 0;
    bool in_token = false;
    for (uint32_t p = s; p < e; p++) {
        const uint8_t b = t[p];
        hi |= b;
        if (is_sep(b)) { in_token = false; continue; }
        if (!in_token) { in_token = true; tokens++; if (tokens == 1) first = b; }
        if (tokens == 1) first_len++;
    }
    if (hi & 0x80) { non_ascii = true; return 0; }
    if (first_len != 1 || tokens < 4) return 0;
    if (first == 'v') return 1;
    if (first == 'f') { tris = tokens - 3; return 2; }
    return 0;
}

// [+-]? digits within int32; false: malformed (an empty part is the caller's case)
YCGE_OBJ_HD bool parse_int(const uint8_t *t, uint32_t a, uint32_t b, int32_t &out)
{
    bool neg = false;
    if (a < b && (t[a] == '+' || t[a] == '-')) { neg = t[a] == '-'; a++; }
    if (a >= b) return false;
    int64_t v = 0;
    uint32_t sig = 0;
    for (; a < b; a++) {
        const uint32_t d = (uint32_t)t[a] - '0';
        if (d > 9) return false;
        if (v == 0 && d == 0) continue;
        if (++sig > 10) return false;
        v = v * 10 + d;
    }
    if (neg) v = -v;
    if (v < INT32_MIN || v > INT32_MAX) return false;
    out = (int32_t)v;
    return true;
}

// one corner token of an `f` line -> its index (ParseIndex); false: malformed
YCGE_OBJ_HD bool parse_corner(const uint8_t *t, uint32_t a, uint32_t b, int32_t count, int32_t &index)
{
    uint32_t cut = a;
    while (cut < b && t[cut] != '/') cut++;
    if (cut == a) { index = 0; return true; }
    int32_t i;
    if (!parse_int(t, a, cut, i)) return false;
    index = i > 0 ? i - 1 : count + i;          // (count >= 0 > i >= -2^31: no overflow)
    return true;
}

// A float token.  0: *out is its correctly rounded binary32; 1: malformed; 2: well formed but outside the EXACT FAST DOMAIN - at most 15
// significant digits w (< 2^53) and a decimal exponent q with |q| <= 22 (10^|q| exact in binary64), or w = 0.  There r = w * 10^q or
// w / 10^-q is ONE correctly rounded binary64 operation on exact operands, r = RN53(v); narrowing r is correct unless r sits exactly on a
// binary32 midpoint (its low 29 bits are 0x10000000) while v does not: the sign of the exact remainder (one fma) then says which way v lies.
// (10^-22 <= v < 10^37: no binary32 overflow or subnormal in the domain.)
YCGE_OBJ_HD int parse_float_fast(const uint8_t *t, uint32_t a, uint32_t b, float *out)
{
    constexpr double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    bool neg = false;
    if (a < b && (t[a] == '+' || t[a] == '-')) { neg = t[a] == '-'; a++; }
    uint64_t w = 0;
    uint32_t sig = 0, int_digits = 0, frac_digits = 0;
    for (; a < b; a++, int_digits++) {
        const uint32_t d = (uint32_t)t[a] - '0';
        if (d > 9) break;
        if (sig == 0 && d == 0) continue;
        if (++sig <= 15) w = w * 10 + d;
    }
    if (a < b && t[a] == '.') {
        for (a++; a < b; a++, frac_digits++) {
            const uint32_t d = (uint32_t)t[a] - '0';
            if (d > 9) break;
            if (sig == 0 && d == 0) continue;
            if (++sig <= 15) w = w * 10 + d;
        }
        if (int_digits == 0 && frac_digits == 0) return 1;
    } else if (int_digits == 0) return 1;
    int32_t ex = 0;
    if (a < b && (t[a] == 'e' || t[a] == 'E')) {
        bool eneg = false;
        a++;
        if (a < b && (t[a] == '+' || t[a] == '-')) { eneg = t[a] == '-'; a++; }
        if (a >= b) return 1;
        for (; a < b; a++) {
            const uint32_t d = (uint32_t)t[a] - '0';
            if (d > 9) return 1;
            if (ex < 100000) ex = ex * 10 + (int32_t)d;
        }
        if (eneg) ex = -ex;
    }
    if (a != b) return 1;
    if (sig == 0) { *out = neg ? -0.0f : 0.0f; return 0; }
    if (sig > 15 || frac_digits > 100000) return 2;
    const int32_t q = ex - (int32_t)frac_digits;
    if (q < -22 || q > 22) return 2;
    const double dw = (double)w, p = p10[q < 0 ? -q : q];
    double r, rem;
    if (q >= 0) { r = dw * p; rem = __builtin_fma(dw, p, -r); }
    else { r = dw / p; rem = __builtin_fma(-r, p, dw); }
    uint64_t bits;
    __builtin_memcpy(&bits, &r, 8);
    if ((bits & 0x1fffffffull) == 0x10000000ull && rem != 0.0) {
        bits += rem > 0.0 ? 1 : -1;
        __builtin_memcpy(&r, &bits, 8);
    }
    const float f = (float)r;
    *out = neg ? -f : f;
    return 0;
}

} // namespace ycge_obj

// ---------------------------------------------------------------------------------------------------------------- the host parser
#include <clocale>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <locale.h>
#include <string>
#include <vector>

namespace ycge_obj {

// status values of include/ycge.h (this header stands alone)
enum { ST_OK = 0, ST_INVALID_ARG = -1, ST_UNSUPPORTED = -4 };

inline std::string error_text(int64_t line, int code)
{
    char buf[160];
    std::snprintf(buf, sizeof buf, "OBJ line %lld: %s", (long long)line,
                  code == BAD_FLOAT ? "malformed float token" : code == BAD_INT ? "malformed integer token"
                                                                                : "a byte >= 0x80 outside a comment (Unicode separators are not supported)");
    return buf;
}
inline const char *empty_text() { return "OBJ had no triangles (no position or no triangle)"; }
inline const char *too_many_text() { return "OBJ has more than 2^28 triangles"; }
inline std::string range_text(int64_t face, int64_t n_positions)
{
    char buf[160];
    std::snprintf(buf, sizeof buf, "OBJ triangle %lld (counted from 0 in file order) names a vertex outside the file's %lld positions", (long long)face, (long long)n_positions);
    return buf;
}
// what every entry refuses of its text argument; 0 or a status
inline int check_text(const uint8_t *text, size_t bytes, std::string &msg)
{
    if (!text || bytes == 0) { msg = "OBJ text is NULL or empty"; return ST_INVALID_ARG; }
    if (bytes >= ((size_t)1 << 31)) { msg = "OBJ text of 2^31 bytes or more"; return ST_INVALID_ARG; }
    return ST_OK;
}

// the value of a float token the grammar accepted: strtof in the C locale (glibc's is correctly rounded for every length and exponent)
inline float float_value(const uint8_t *t, uint32_t a, uint32_t b, std::string &scratch)
{
    static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    scratch.assign((const char *)t + a, (const char *)t + b);
    return c_locale ? strtof_l(scratch.c_str(), nullptr, c_locale) : strtof(scratch.c_str(), nullptr);
}

// positions (3 per vertex) and faces (3 per triangle) of `text`; 0 or a status with its message, the arrays then unspecified
inline int parse_host(const uint8_t *text, size_t bytes, std::vector<float> &pos, std::vector<int32_t> &faces, int64_t &n_lines, std::string &msg)
{
    pos.clear(); faces.clear(); n_lines = 0;
    { const int rc = check_text(text, bytes, msg); if (rc != ST_OK) return rc; }
    const uint32_t n = (uint32_t)bytes;
    uint32_t p = n >= 3 && text[0] == 0xef && text[1] == 0xbb && text[2] == 0xbf ? 3u : 0u;
    int64_t n_tris = 0;
    std::string scratch;
    while (p < n) {
        n_lines++;
        uint32_t e = p;
        while (e < n && text[e] != '\n' && text[e] != '\r') e++;
        uint32_t tris;
        bool non_ascii;
        const int kind = classify_line(text, p, e, tris, non_ascii);
        if (non_ascii) { msg = error_text(n_lines, NON_ASCII); return ST_UNSUPPORTED; }
        uint32_t q = p, a, b;
        if (kind == 1) {
            (void)next_token(text, q, e, a, b);
            for (int k = 0; k < 3; k++) {
                (void)next_token(text, q, e, a, b);
                float ignored;
                if (parse_float_fast(text, a, b, &ignored) == 1) { msg = error_text(n_lines, BAD_FLOAT); return ST_INVALID_ARG; }
                pos.push_back(float_value(text, a, b, scratch));
            }
        } else if (kind == 2) {
            (void)next_token(text, q, e, a, b);
            const int32_t count = (int32_t)(pos.size() / 3);
            int32_t v0 = 0, prev = 0;
            for (uint32_t k = 0; next_token(text, q, e, a, b); k++) {
                int32_t idx;
                if (!parse_corner(text, a, b, count, idx)) { msg = error_text(n_lines, BAD_INT); return ST_INVALID_ARG; }
                if (k == 0) v0 = idx;
                else if (k >= 2 && ++n_tris <= kMaxTriangles) { faces.push_back(v0); faces.push_back(prev); faces.push_back(idx); }
                prev = idx;
            }
        }
        p = e;
        if (p < n) p += text[p] == '\r' && p + 1 < n && text[p + 1] == '\n' ? 2 : 1;
    }
    if (n_tris > kMaxTriangles) { msg = too_many_text(); return ST_INVALID_ARG; }
    if (pos.empty() || faces.empty()) { msg = empty_text(); return ST_INVALID_ARG; }
    const int64_t nv = (int64_t)(pos.size() / 3);
    for (size_t k = 0; k < faces.size(); k++)
        if (faces[k] < 0 || faces[k] >= nv) { msg = range_text((int64_t)(k / 3), nv); return ST_INVALID_ARG; }
    return ST_OK;
}

} // namespace ycge_obj

// ---------------------------------------------------------------------------------------------------------------- the auto-ground tail
// MeshScenes.TryReadObjBoundsNormalized behind its parse (Scenes/MeshScenes.cs:233-330) on parsed arrays: ycge_obj_ground_host, the
// yardstick of the kernels of ycge_obj_ground.hip and their fallback.  THE CONTRACT (tests/obj_ground_restatement.py states it again):
//   components  vertices joined by the edges (a, b) and (b, c) of every face; which vertex is a root never reaches the result
//   the chosen  the component with the most faces; among equal counts the one whose first face comes first in file order
//   centroid    cx = 0; per kept face in file order cx += ((A.x + B.x) + C.x) * (1 / 3f), every operation rounded to binary32 (no contracted
//               multiply-add: compile without contraction); then cx *= 1 / (float)kept.  y and z alike
//   bounds      over the vertices of the kept faces, of pos - centroid; NaN never replaces an extreme; -0 orders below +0
//   normalise   extent = rx; if (ry > extent); if (rz > extent); if (extent <= 0) extent = 1; s = 1 / extent; min = rMin * s; max = rMax * s
namespace ycge_obj {

// ycge_obj_ground_info of include/ycge.h, field for field (this header stands alone; ycge_obj.cpp asserts the size)
struct GroundInfo {
    float min[3], max[3], centroid[3], extent;
    int32_t n_components, component_faces, component_vertices, first_face, on_device, reserved;
};
// why the kernels did not take the tail (ycge_debug_obj_ground_stats, out6[2]); the kernels set the first two
enum { GROUND_DECLINE_FIND_BOUND = 1, GROUND_DECLINE_ROUND_CAP = 2, GROUND_DECLINE_ENV_HOST = 4, GROUND_DECLINE_BELOW_MIN = 8 };
constexpr int kGroundRoundCap = 64;                  // labelling rounds before the host tail takes the OBJ

// a float as an unsigned integer of the same order (-0 below +0): the order the kernels' min / max use
inline uint32_t ground_ordered(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// steps 5 of the contract: raw extremes about the centroid -> out.extent, out.min, out.max
inline void ground_normalise(const float rmin[3], const float rmax[3], GroundInfo &out)
{
    const float rx = rmax[0] - rmin[0], ry = rmax[1] - rmin[1], rz = rmax[2] - rmin[2];
    float extent = rx;
    if (ry > extent) extent = ry;
    if (rz > extent) extent = rz;
    if (extent <= 0.0f) extent = 1.0f;
    const float s = 1.0f / extent;
    out.extent = extent;
    for (int a = 0; a < 3; a++) { out.min[a] = rmin[a] * s; out.max[a] = rmax[a] * s; }
}

// 0 or ST_INVALID_ARG (NULL arrays, counts <= 0, an index out of range)
inline int ground_host(const float *positions, int32_t n_positions, const int32_t *faces, int32_t n_triangles, GroundInfo &out)
{
    std::memset(&out, 0, sizeof out);
    if (!positions || !faces || n_positions <= 0 || n_triangles <= 0) return ST_INVALID_ARG;
    const size_t nv = (size_t)n_positions, nf = (size_t)n_triangles;
    for (size_t k = 0; k < 3 * nf; k++)
        if (faces[k] < 0 || faces[k] >= n_positions) return ST_INVALID_ARG;
    // union-find, the larger root under the smaller (no rank: the root's identity is not part of the result), path halving
    std::vector<int32_t> parent(nv);
    for (size_t v = 0; v < nv; v++) parent[v] = (int32_t)v;
    auto find = [&](int32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    auto join = [&](int32_t x, int32_t y) { const int32_t a = find(x), b = find(y); if (a < b) parent[b] = a; else if (b < a) parent[a] = b; };
    for (size_t f = 0; f < nf; f++) { join(faces[3 * f], faces[3 * f + 1]); join(faces[3 * f + 1], faces[3 * f + 2]); }
    // faces per root; the winner: strictly more faces in order of first appearance (the Dictionary's insertion order)
    std::vector<int32_t> count(nv, 0), root_of(nf);
    int32_t best = -1, best_first = 0, n_components = 0;
    for (size_t f = 0; f < nf; f++) { const int32_t r = find(faces[3 * f]); root_of[f] = r; if (count[r]++ == 0) n_components++; }
    {
        std::vector<uint8_t> seen(nv, 0);
        for (size_t f = 0; f < nf; f++) {
            const int32_t r = root_of[f];
            if (seen[r]) continue;
            seen[r] = 1;
            if (best < 0 || count[r] > count[best]) { best = r; best_first = (int32_t)f; }
        }
    }
    const float third = 1.0f / 3.0f;
    float c[3] = {0.0f, 0.0f, 0.0f};
    std::vector<uint8_t> used(nv, 0);
    for (size_t f = 0; f < nf; f++) {
        if (root_of[f] != best) continue;
        const size_t ia = (size_t)faces[3 * f], ib = (size_t)faces[3 * f + 1], ic = (size_t)faces[3 * f + 2];
        used[ia] = used[ib] = used[ic] = 1;
        for (int a = 0; a < 3; a++) {
            const float sum = (positions[3 * ia + a] + positions[3 * ib + a]) + positions[3 * ic + a];
            const float term = sum * third;          // (rounded before it is added)
            c[a] = c[a] + term;
        }
    }
    const float inv = 1.0f / (float)count[best];
    for (int a = 0; a < 3; a++) c[a] = c[a] * inv;
    float rmin[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, rmax[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int32_t n_used = 0;
    for (size_t v = 0; v < nv; v++) {
        if (!used[v]) continue;
        n_used++;
        for (int a = 0; a < 3; a++) {
            const float x = positions[3 * v + a] - c[a];
            if (x != x) continue;
            if (ground_ordered(x) < ground_ordered(rmin[a])) rmin[a] = x;
            if (ground_ordered(x) > ground_ordered(rmax[a])) rmax[a] = x;
        }
    }
    for (int a = 0; a < 3; a++) out.centroid[a] = c[a];
    ground_normalise(rmin, rmax, out);
    out.n_components = n_components; out.component_faces = count[best]; out.component_vertices = n_used; out.first_face = best_first;
    return ST_OK;
}

} // namespace ycge_obj
