// ycge_obj.hip - MeshLoader.FromObj on the device (host side: ycge_obj.cpp; the reading rules and their token routines: ycge_obj.h).
//
// Where a line starts is a local function of two neighbouring bytes, what a line adds (a position, tokens - 3 triangles) is a local function
// of the line, and where it writes is an exclusive prefix sum: reduce-then-scan over tiles, twice, as ycge_ansi.hip is built.
//   k_obj_mark<false>  per tile of kObjTile bytes: its line starts, counted              k_obj_scan: the tiles' offsets, the line count
//   k_obj_mark<true>   the starts again, compacted into the line table
//   k_obj_classify     one lane, one line: kind, positions and triangles it adds; per workgroup of kObjBlock lines their sums
//   k_obj_scan (x2)    the workgroups' offsets, the position and triangle counts
//   k_obj_parse        the same walk, writing: a `v` line its position, an `f` line its fan; errors to one 64-bit word by atomicMin of
//                      (line << 8 | code) - the lowest line wins whatever the order of arrival; declines to a flag word
//   k_obj_used         faces mark used[]; an index out of range reports the lowest triangle through a second error word
//   k_obj_bounds       min / max over the used vertices: per workgroup in LDS, then one ordered-integer atomic per workgroup and component
//   k_obj_triangles    one lane, one triangle: gather, normalise, scale / translate, store; its bounds by the same two-stage reduction
//                      (ycge_obj_box.hip.h, shared with ycge_obj_ground.hip)
// Float min / max are exact, so the order of arrival cannot change a bit; -0 orders below +0 here (the reference's sign of a zero extreme
// depends on HashSet enumeration order), NaN never replaces an extreme (the reference's compares are false for it).
// No workgroup waits on another's flag.  Lanes take lines of different lengths, so the walk diverges: accepted for this first form (nothing
// about its rate against the upload has been measured yet, profiles/obj_rate.py).  Offsets are 32-bit: the host refuses 2^31 bytes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_obj.h"
#include "ycge_obj_box.hip.h"

namespace {

using namespace ycge_obj;

constexpr int kObjBlock = 256;
constexpr int kObjPerLane = 16;                                   // bytes of text per lane of k_obj_mark: one 16-byte load
constexpr int kObjTile = kObjBlock * kObjPerLane;

// header words the kernels write (ObjHeader of ycge_obj.cpp reads them back)
struct ObjHeader {
    unsigned long long err;               // lowest (line << 8 | code), ~0 = none
    unsigned long long bad_face;          // lowest triangle with an index out of range, ~0 = none
    uint32_t decline;                     // DECLINE_* bits
    uint32_t n_lines, n_positions, n_triangles;
    uint32_t used_box[6];                 // ordered-integer min xyz, max xyz over the used vertices
    uint32_t tri_box[6];                  // ... over the corners of the last triangle pass
};

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
    for (int w = 0; w < kObjBlock / 64; w++) {
        const uint32_t s = wsum[w];
        before += w < wid ? s : 0u;
        total += s;
    }
    __syncthreads();                      // (wsum may be reused)
    return before + inc - v;
}

// bit k: byte base + k of the text starts a line.  first: 0, or 3 behind a byte-order mark.  The text buffer is readable up to the next
// multiple of 16 bytes past n (the host allocates it so); bytes at or past n are never interpreted.
__device__ __forceinline__ uint32_t line_start_mask(const uint8_t *__restrict__ text, uint32_t n, uint32_t first, uint32_t base)
{
    if (base >= n) return 0u;
    const uint4 q = *reinterpret_cast<const uint4 *>(text + base);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t prev = base > 0 ? text[base - 1] : 0u, mask = 0u;
#pragma unroll
    for (int k = 0; k < kObjPerLane; k++) {
        const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xffu, p = base + (uint32_t)k;
        const bool start = p < n && (p == first || (p > first && (prev == '\n' || (prev == '\r' && b != '\n'))));
        mask |= start ? 1u << k : 0u;
        prev = b;
    }
    return mask;
}

template <bool kWrite>
__global__ __launch_bounds__(kObjBlock) void k_obj_mark(const uint8_t *__restrict__ text, uint32_t n, uint32_t first, uint32_t *__restrict__ tiles,
                                                         uint32_t *__restrict__ line_start, uint32_t n_lines)
{
    __shared__ uint32_t wsum[kObjBlock / 64];
    const uint32_t base = blockIdx.x * (uint32_t)kObjTile + threadIdx.x * (uint32_t)kObjPerLane;
    uint32_t mask = line_start_mask(text, n, first, base);
    uint32_t total;
    uint32_t at = block_exclusive_scan((uint32_t)__popc(mask), wsum, total);
    if (!kWrite) {
        if (threadIdx.x == 0) tiles[blockIdx.x] = total;
        return;
    }
    at += tiles[blockIdx.x];
    for (; mask; mask &= mask - 1u, at++)
        if (at < n_lines) line_start[at] = base + (uint32_t)__ffs(mask) - 1u;
}

// one workgroup: v[0 .. m) -> exclusive offsets in place, the sum to *total
__global__ __launch_bounds__(kObjBlock) void k_obj_scan(uint32_t *__restrict__ v, uint32_t m, uint32_t *__restrict__ total_out)
{
    __shared__ uint32_t wsum[kObjBlock / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < m; base += kObjBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t x = t < m ? v[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(x, wsum, total);
        if (t < m) v[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// the line i of the table: [s, e) without its terminator
__device__ __forceinline__ void line_span(const uint8_t *__restrict__ text, uint32_t n, const uint32_t *__restrict__ line_start, uint32_t n_lines, uint32_t i,
                                          uint32_t &s, uint32_t &e)
{
    s = line_start[i];
    e = i + 1u < n_lines ? line_start[i + 1u] : n;
    if (e > s && text[e - 1u] == '\n') e--;
    if (e > s && text[e - 1u] == '\r') e--;
}

// add[i] = positions (bit 31) and triangles (bits 0..30) line i adds; block_pos / block_tri: the sums over each workgroup's lines
__global__ __launch_bounds__(kObjBlock) void k_obj_classify(const uint8_t *__restrict__ text, uint32_t n, const uint32_t *__restrict__ line_start, uint32_t n_lines,
                                                             uint32_t *__restrict__ add, uint32_t *__restrict__ block_pos, uint32_t *__restrict__ block_tri,
                                                             ObjHeader *__restrict__ H)
{
    __shared__ uint32_t wsum[kObjBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kObjBlock + threadIdx.x;
    uint32_t pos = 0, tris = 0;
    if (i < n_lines) {
        uint32_t s, e;
        line_span(text, n, line_start, n_lines, i, s, e);
        if (e - s > kLineCap && text[s] != '#') atomicOr(&H->decline, (uint32_t)DECLINE_LINE_CAP);
        else {
            bool non_ascii;
            const int kind = classify_line(text, s, e, tris, non_ascii);
            if (non_ascii) atomicMin(&H->err, ((unsigned long long)(i + 1u) << 8) | (unsigned long long)NON_ASCII);
            pos = kind == 1 ? 1u : 0u;
        }
        add[i] = (pos << 31) | tris;
    }
    uint32_t total;
    (void)block_exclusive_scan(pos, wsum, total);
    if (threadIdx.x == 0) block_pos[blockIdx.x] = total;
    (void)block_exclusive_scan(tris, wsum, total);
    if (threadIdx.x == 0) block_tri[blockIdx.x] = total;
}

// positions == NULL: nothing is written, the tokens are checked all the same (a file of too many triangles still names its first bad line)
__global__ __launch_bounds__(kObjBlock) void k_obj_parse(const uint8_t *__restrict__ text, uint32_t n, const uint32_t *__restrict__ line_start, uint32_t n_lines,
                                                          const uint32_t *__restrict__ add, const uint32_t *__restrict__ block_pos, const uint32_t *__restrict__ block_tri,
                                                          float *__restrict__ positions, int32_t *__restrict__ faces, uint32_t n_positions, uint32_t n_triangles,
                                                          ObjHeader *__restrict__ H)
{
    __shared__ uint32_t wsum[kObjBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kObjBlock + threadIdx.x;
    const uint32_t mine = i < n_lines ? add[i] : 0u;
    uint32_t total;
    const uint32_t pos_at = block_pos[blockIdx.x] + block_exclusive_scan(mine >> 31, wsum, total);
    uint32_t tri_at = block_tri[blockIdx.x] + block_exclusive_scan(mine & 0x7fffffffu, wsum, total);
    if (mine == 0u) return;
    uint32_t s, e, a, b;
    line_span(text, n, line_start, n_lines, i, s, e);
    const unsigned long long line_key = (unsigned long long)(i + 1u) << 8;
    uint32_t p = s;
    (void)next_token(text, p, e, a, b);                                  // "v" / "f"
    if (mine >> 31) {
        float xyz[3];
        for (int k = 0; k < 3; k++) {
            (void)next_token(text, p, e, a, b);
            const int rc = parse_float_fast(text, a, b, &xyz[k]);
            if (rc == 1) { atomicMin(&H->err, line_key | (unsigned long long)BAD_FLOAT); return; }
            if (rc == 2) { atomicOr(&H->decline, (uint32_t)DECLINE_FLOAT_DOMAIN); return; }
        }
        if (positions && pos_at < n_positions) { positions[3 * (size_t)pos_at] = xyz[0]; positions[3 * (size_t)pos_at + 1] = xyz[1]; positions[3 * (size_t)pos_at + 2] = xyz[2]; }
        return;
    }
    int32_t v0 = 0, prev = 0;
    for (uint32_t k = 0; next_token(text, p, e, a, b); k++) {
        int32_t idx;
        if (!parse_corner(text, a, b, (int32_t)pos_at, idx)) { atomicMin(&H->err, line_key | (unsigned long long)BAD_INT); return; }
        if (k == 0) v0 = idx;
        else if (k >= 2) {
            if (faces && tri_at < n_triangles) { faces[3 * (size_t)tri_at] = v0; faces[3 * (size_t)tri_at + 1] = prev; faces[3 * (size_t)tri_at + 2] = idx; }
            tri_at++;
        }
        prev = idx;
    }
}

__global__ __launch_bounds__(kObjBlock) void k_obj_used(const int32_t *__restrict__ faces, uint32_t n_triangles, uint32_t n_positions, uint8_t *__restrict__ used,
                                                         ObjHeader *__restrict__ H)
{
    const uint32_t f = blockIdx.x * (uint32_t)kObjBlock + threadIdx.x;
    if (f >= n_triangles) return;
    bool bad = false;
    for (int k = 0; k < 3; k++) {
        const int32_t v = faces[3 * (size_t)f + k];
        if (v < 0 || (uint32_t)v >= n_positions) bad = true;
        else used[v] = 1;
    }
    if (bad) atomicMin(&H->bad_face, (unsigned long long)f);
}

__global__ __launch_bounds__(kObjBlock) void k_obj_bounds(const float *__restrict__ positions, uint32_t n_positions, const uint8_t *__restrict__ used, ObjHeader *__restrict__ H)
{
    const uint32_t v = blockIdx.x * (uint32_t)kObjBlock + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (v < n_positions && used[v]) {
        const float p[3] = {positions[3 * (size_t)v], positions[3 * (size_t)v + 1], positions[3 * (size_t)v + 2]};
        grow(lo, hi, p);
    }
    reduce_box(lo, hi, H->used_box);
}

struct ObjTail {
    int32_t normalize, transform;
    float c[3], s, scale, t[3];
};

__global__ __launch_bounds__(kObjBlock) void k_obj_triangles(const float *__restrict__ positions, const int32_t *__restrict__ faces, uint32_t n_triangles, ObjTail T,
                                                              float *__restrict__ out, ObjHeader *__restrict__ H)
{
    const uint32_t f = blockIdx.x * (uint32_t)kObjBlock + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (f < n_triangles) {
        for (int k = 0; k < 3; k++) {
            const size_t v = (size_t)faces[3 * (size_t)f + k];           // (in range: the parse refused the file otherwise)
            float p[3] = {positions[3 * v], positions[3 * v + 1], positions[3 * v + 2]};
            if (T.normalize) for (int a = 0; a < 3; a++) p[a] = (p[a] - T.c[a]) * T.s;
            if (T.transform) for (int a = 0; a < 3; a++) p[a] = p[a] * T.scale + T.t[a];
            for (int a = 0; a < 3; a++) out[9 * (size_t)f + 3 * k + a] = p[a];
            grow(lo, hi, p);
        }
    }
    reduce_box(lo, hi, H->tri_box);
}

inline uint32_t blocks_of(uint32_t n, uint32_t per) { return (n + per - 1u) / per; }

} // namespace

// bytes of the header the launchers share, and the geometry the tests size their files by: 0 header bytes, 1 the mark kernel's tile in bytes,
// 2 the lines one workgroup of the line kernels takes, 3 the line cap in bytes
extern "C" size_t ycge_launch_obj_sizes(int which)
{
    return which == 0 ? sizeof(ObjHeader) : which == 1 ? (size_t)kObjTile : which == 2 ? (size_t)kObjBlock : which == 3 ? (size_t)ycge_obj::kLineCap : 0;
}

// stage 1: the header cleared, the tiles' line starts counted and scanned; header.n_lines.  text: n bytes, readable to the next multiple of
// 16; tiles: ceil(n / tile) words
extern "C" int ycge_launch_obj_count_lines(const uint8_t *text, uint32_t n, uint32_t first, uint32_t *tiles, void *header, hipStream_t stream)
{
    if (!text || !tiles || !header || n == 0 || n >= 0x80000000u || first > 3u) return (int)hipErrorInvalidValue;
    ObjHeader *H = static_cast<ObjHeader *>(header);
    hipError_t e = hipMemsetAsync(H, 0xff, 16, stream);                       // err, bad_face: none
    if (e == hipSuccess) e = hipMemsetAsync(&H->decline, 0, sizeof(ObjHeader) - 16, stream);
    if (e != hipSuccess) return (int)e;
    const uint32_t n_tiles = blocks_of(n, kObjTile);
    hipLaunchKernelGGL(k_obj_mark<false>, dim3(n_tiles), dim3(kObjBlock), 0, stream, text, n, first, tiles, (uint32_t *)nullptr, 0u);
    hipLaunchKernelGGL(k_obj_scan, dim3(1), dim3(kObjBlock), 0, stream, tiles, n_tiles, &H->n_lines);
    return (int)hipGetLastError();
}

// stage 2: the line table (n_lines words), what each line adds (add: n_lines words), the workgroups' offsets (block_pos, block_tri:
// ceil(n_lines / lines per workgroup) words each); header.n_positions, n_triangles, err (non-ASCII lines), decline (line cap)
extern "C" int ycge_launch_obj_classify(const uint8_t *text, uint32_t n, uint32_t first, const uint32_t *tiles, uint32_t *line_start, uint32_t n_lines, uint32_t *add,
                                        uint32_t *block_pos, uint32_t *block_tri, void *header, hipStream_t stream)
{
    if (!text || !tiles || !line_start || !add || !block_pos || !block_tri || !header || n_lines == 0) return (int)hipErrorInvalidValue;
    ObjHeader *H = static_cast<ObjHeader *>(header);
    const uint32_t n_blocks = blocks_of(n_lines, kObjBlock);
    hipLaunchKernelGGL(k_obj_mark<true>, dim3(blocks_of(n, kObjTile)), dim3(kObjBlock), 0, stream, text, n, first, const_cast<uint32_t *>(tiles), line_start, n_lines);
    hipLaunchKernelGGL(k_obj_classify, dim3(n_blocks), dim3(kObjBlock), 0, stream, text, n, (const uint32_t *)line_start, n_lines, add, block_pos, block_tri, H);
    hipLaunchKernelGGL(k_obj_scan, dim3(1), dim3(kObjBlock), 0, stream, block_pos, n_blocks, &H->n_positions);
    hipLaunchKernelGGL(k_obj_scan, dim3(1), dim3(kObjBlock), 0, stream, block_tri, n_blocks, &H->n_triangles);
    return (int)hipGetLastError();
}

// stage 3: positions (3 n_positions floats) and faces (3 n_triangles int32), or the token check alone (both NULL); header.err, decline
extern "C" int ycge_launch_obj_parse(const uint8_t *text, uint32_t n, const uint32_t *line_start, uint32_t n_lines, const uint32_t *add, const uint32_t *block_pos,
                                     const uint32_t *block_tri, float *positions, int32_t *faces, uint32_t n_positions, uint32_t n_triangles, void *header, hipStream_t stream)
{
    if (!text || !line_start || !add || !block_pos || !block_tri || !header || n_lines == 0 || (positions == nullptr) != (faces == nullptr)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_obj_parse, dim3(blocks_of(n_lines, kObjBlock)), dim3(kObjBlock), 0, stream, text, n, line_start, n_lines, add, block_pos, block_tri, positions, faces,
                       n_positions, n_triangles, static_cast<ObjHeader *>(header));
    return (int)hipGetLastError();
}

// stage 4: used (n_positions bytes, cleared here), header.bad_face, header.used_box
extern "C" int ycge_launch_obj_used_bounds(const float *positions, const int32_t *faces, uint32_t n_positions, uint32_t n_triangles, uint8_t *used, void *header, hipStream_t stream)
{
    if (!positions || !faces || !used || !header || n_positions == 0 || n_triangles == 0) return (int)hipErrorInvalidValue;
    ObjHeader *H = static_cast<ObjHeader *>(header);
    hipError_t e = hipMemsetAsync(used, 0, n_positions, stream);
    if (e == hipSuccess) e = hipMemsetAsync(&H->used_box[0], 0xff, 12, stream);
    if (e == hipSuccess) e = hipMemsetAsync(&H->used_box[3], 0, 12, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_obj_used, dim3(blocks_of(n_triangles, kObjBlock)), dim3(kObjBlock), 0, stream, faces, n_triangles, n_positions, used, H);
    hipLaunchKernelGGL(k_obj_bounds, dim3(blocks_of(n_positions, kObjBlock)), dim3(kObjBlock), 0, stream, positions, n_positions, (const uint8_t *)used, H);
    return (int)hipGetLastError();
}

// stage 5: out (9 n_triangles floats) and header.tri_box.  c, s: NormalizeAllUsedVertices' centre and factor (read when normalize != 0);
// scale, t: read when transform != 0.  Every index of faces is in range.
extern "C" int ycge_launch_obj_triangles(const float *positions, const int32_t *faces, uint32_t n_triangles, int normalize, const float c[3], float s, int transform,
                                         float scale, const float t[3], float *out, void *header, hipStream_t stream)
{
    if (!positions || !faces || !out || !header || !c || !t || n_triangles == 0) return (int)hipErrorInvalidValue;
    ObjHeader *H = static_cast<ObjHeader *>(header);
    hipError_t e = hipMemsetAsync(&H->tri_box[0], 0xff, 12, stream);
    if (e == hipSuccess) e = hipMemsetAsync(&H->tri_box[3], 0, 12, stream);
    if (e != hipSuccess) return (int)e;
    ObjTail T;
    T.normalize = normalize; T.transform = transform; T.s = s; T.scale = scale;
    for (int a = 0; a < 3; a++) { T.c[a] = c[a]; T.t[a] = t[a]; }
    hipLaunchKernelGGL(k_obj_triangles, dim3(blocks_of(n_triangles, kObjBlock)), dim3(kObjBlock), 0, stream, positions, faces, n_triangles, T, out, H);
    return (int)hipGetLastError();
}
