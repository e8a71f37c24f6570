// ycge_obj_ground.hip - MeshScenes.TryReadObjBoundsNormalized behind its parse (Scenes/MeshScenes.cs:233-330) on the held OBJ: the
// component with the most faces, its centroid, the bounds of its vertices about that centroid (host side: ycge_obj.cpp, obj_ground; the
// contract and the host tail that is its yardstick and fallback: ycge_obj.h).
//
//   k_ground_init      parent[v] = v
//   k_ground_hook      one lane, one face: its edges (a, b), (b, c) joined in a lock-free union-find - the LARGER root is hooked under the
//                      SMALLER by atomicCAS, a failed CAS continues from the value it returned.  parent[v] <= v always, and only ever
//                      falls: a walk towards the root strictly descends, so it ends within n_positions steps whatever it reads, and a
//                      component's final root is its LOWEST vertex index - nothing of the result depends on scheduling.
//   k_ground_flatten   parent[v] = root(v)
//                      The device's eight XCDs have private L2s and a plain load may return another XCD's stale line inside one launch
//                      (profiles/micro/xcdvis.hip): EVERY access to parent[] in these two kernels is an agent-scope atomic (relaxed loads,
//                      atomicCAS, atomicMin).  On top of that the host repeats hook + flatten until a round hooks nothing: that last round
//                      reads only what earlier LAUNCHES wrote, and it proves every edge lies inside one tree.  A clean run takes two rounds.
//   k_ground_count     faces per root (atomicAdd) and each root's first face (atomicMin); lanes of a wavefront that share the root of its
//                      first lane go through one atomic (one component usually owns almost every face)
//   k_ground_winner    one 64-bit atomicMax of (count << 32 | ~first_face) over the roots that own a face: the most faces, then the lowest
//                      first face - the first strictly larger count in the Dictionary's insertion order
//   k_ground_terms     one lane, one face, three planes: term[f] = kept ? ((A + B) + C) * (1 / 3f) : +0.  Adding +0 leaves every value the
//                      running sum can take unchanged (it starts at +0 and x + (-x) is +0 under round-to-nearest, so it is never -0):
//                      no compaction is needed.  The argument of k_exposure_terms (ycge_post.hip).  Kept faces mark used[].
//   k_ground_sum       cx += term in file order by ONE lane per axis, three workgroups side by side: k_exposure_sum_serial's hand-pipelined
//                      chain (ycge_post.hip: 6.5 cycles per add); then centroid = sum * (1 / (float)kept)
//   k_ground_bounds    min / max of pos - centroid over the used vertices (ycge_obj_box.hip.h), the used vertices counted
// No workgroup waits on another's flag.  Every loop has a bound the host can state: a walk n_positions steps, a hook n_positions retries
// (each retry starts strictly lower), the rounds kGroundRoundCap; past a bound a decline bit is set and the host tail takes the OBJ.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_obj.h"
#include "ycge_obj_box.hip.h"

namespace {

using namespace ycge_obj;

constexpr int kGroundBlock = 256;
constexpr uint32_t kGroundChunk = 1024;               // terms one trip of k_ground_sum takes: the planes are padded to a multiple with +0
constexpr uint32_t kNoRoot = 0xffffffffu;

// what the kernels report (GroundHeaderHost of ycge_obj.cpp reads it back)
struct GroundHeader {
    unsigned long long best;              // (faces << 32 | ~first face) of the chosen component
    uint32_t decline, changed;            // GROUND_DECLINE_* bits; != 0: the last round hooked something
    uint32_t n_components, n_used;
    uint32_t box[6];                      // ordered-integer min xyz, max xyz of pos - centroid over the used vertices
    float sum[3], centroid[3];
    uint32_t pad[2];
};

__device__ __forceinline__ uint32_t parent_of(const uint32_t *parent, uint32_t x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x, halving the path on the way (the writes only lower a parent); kNoRoot: more than `bound` steps
__device__ __forceinline__ uint32_t find_root(uint32_t *parent, uint32_t x, uint32_t bound)
{
    uint32_t p = parent_of(parent, x);
    for (uint32_t steps = 0; p != x; steps++) {
        if (steps >= bound) return kNoRoot;
        const uint32_t g = parent_of(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// true: this call hooked a root; bad: a bound was passed
__device__ __forceinline__ bool hook(uint32_t *parent, uint32_t a, uint32_t b, uint32_t bound, bool &bad)
{
    uint32_t ra = find_root(parent, a, bound), rb = find_root(parent, b, bound);
    for (uint32_t tries = 0;; tries++) {
        if (ra == kNoRoot || rb == kNoRoot || tries > bound) { bad = true; return false; }
        if (ra == rb) return false;
        const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return true;
        ra = find_root(parent, old, bound);          // (hi is a root no longer: on from what it hangs under now; old < hi)
        rb = find_root(parent, lo, bound);
    }
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_init(uint32_t *__restrict__ parent, uint32_t n_positions)
{
    const uint32_t v = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    if (v < n_positions) parent[v] = v;
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_hook(const int32_t *__restrict__ faces, uint32_t n_triangles, uint32_t n_positions, uint32_t *parent, GroundHeader *H)
{
    const uint32_t f = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    bool changed = false, bad = false;
    if (f < n_triangles) {
        const uint32_t a = (uint32_t)faces[3 * (size_t)f], b = (uint32_t)faces[3 * (size_t)f + 1], c = (uint32_t)faces[3 * (size_t)f + 2];   // (in range: the parse refused the file otherwise)
        changed = hook(parent, a, b, n_positions, bad);
        changed |= hook(parent, b, c, n_positions, bad);
    }
    if (changed) atomicOr(&H->changed, 1u);
    if (bad) atomicOr(&H->decline, (uint32_t)GROUND_DECLINE_FIND_BOUND);
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_flatten(uint32_t *parent, uint32_t n_positions, GroundHeader *H)
{
    const uint32_t v = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    if (v >= n_positions) return;
    const uint32_t r = find_root(parent, v, n_positions);
    if (r == kNoRoot) atomicOr(&H->decline, (uint32_t)GROUND_DECLINE_FIND_BOUND);
    else atomicMin(parent + v, r);
}

// parent[] is flat from here on, and written by earlier launches only
__global__ __launch_bounds__(kGroundBlock) void k_ground_count(const int32_t *__restrict__ faces, uint32_t n_triangles, const uint32_t *__restrict__ parent,
                                                                uint32_t *__restrict__ count, uint32_t *__restrict__ first)
{
    const uint32_t f = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    const bool live = f < n_triangles;
    const uint32_t r = live ? parent[(uint32_t)faces[3 * (size_t)f]] : kNoRoot;
    const uint32_t r0 = (uint32_t)__shfl((int)r, 0, 64);          // (faces ascend with the lane: the first lane is live when any is, and its face is the wavefront's lowest)
    const unsigned long long same = __ballot(live && r == r0);
    if (!live) return;
    if (r != r0) { atomicAdd(count + r, 1u); atomicMin(first + r, f); }
    else if ((threadIdx.x & 63) == 0) { atomicAdd(count + r0, (uint32_t)__popcll(same)); atomicMin(first + r0, f); }
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_winner(const uint32_t *__restrict__ count, const uint32_t *__restrict__ first, uint32_t n_positions, GroundHeader *H)
{
    const uint32_t v = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    if (v >= n_positions) return;
    const uint32_t n = count[v];
    if (n == 0u) return;
    atomicMax(&H->best, ((unsigned long long)n << 32) | (unsigned long long)(uint32_t)~first[v]);
    atomicAdd(&H->n_components, 1u);
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_terms(const float *__restrict__ positions, const int32_t *__restrict__ faces, uint32_t n_triangles, uint32_t padded,
                                                                const uint32_t *__restrict__ parent, const GroundHeader *__restrict__ H, float *__restrict__ terms,
                                                                uint8_t *__restrict__ used)
{
    const uint32_t f = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    if (f >= padded) return;
    float t[3] = {0.0f, 0.0f, 0.0f};
    if (f < n_triangles) {
        const uint32_t first_face = ~(uint32_t)H->best;
        const uint32_t root = first_face < n_triangles ? parent[(uint32_t)faces[3 * (size_t)first_face]] : kNoRoot;          // (always a face: at least one root owns one)
        const uint32_t ia = (uint32_t)faces[3 * (size_t)f], ib = (uint32_t)faces[3 * (size_t)f + 1], ic = (uint32_t)faces[3 * (size_t)f + 2];
        if (parent[ia] == root) {
            const float third = 1.0f / 3.0f;
            for (int a = 0; a < 3; a++)
                t[a] = __fmul_rn(__fadd_rn(__fadd_rn(positions[3 * (size_t)ia + a], positions[3 * (size_t)ib + a]), positions[3 * (size_t)ic + a]), third);
            used[ia] = 1; used[ib] = 1; used[ic] = 1;
        }
    }
    for (int a = 0; a < 3; a++) terms[(size_t)a * padded + f] = t[a];
}

// One workgroup (one wavefront) per axis.  The adds are ONE dependent chain and nothing else may sit on it: the wavefront fetches the next
// 1024 terms with coalesced 16-byte loads while lane 0 adds the current 1024 out of LDS, 32 terms in registers (set A) while the next 32
// (set B) are on their way out of LDS - reads issued by hand (ds_read_b128, no wait), consumed behind an explicit s_waitcnt that leaves the
// OTHER set's eight reads outstanding.  The loop of k_exposure_sum_serial (ycge_post.hip), where it was measured.
__global__ __launch_bounds__(64) void k_ground_sum(const float *__restrict__ terms, uint32_t padded, GroundHeader *H)
{
    __shared__ float4 s_buf[2][256];
    const int lane = threadIdx.x;
    const float4 *t4 = (const float4 *)(terms + (size_t)blockIdx.x * padded);
    const uint32_t n_chunks = padded / kGroundChunk;
    float sum = 0.0f;
    float4 r0, r1, r2, r3;
    if (n_chunks > 0) { r0 = t4[lane]; r1 = t4[64 + lane]; r2 = t4[128 + lane]; r3 = t4[192 + lane]; }
    for (uint32_t c = 0; c < n_chunks; c++) {
        float4 *buf = s_buf[c & 1];
        buf[lane] = r0; buf[64 + lane] = r1; buf[128 + lane] = r2; buf[192 + lane] = r3;
        if (c + 1 < n_chunks) {
            const float4 *nx = t4 + (size_t)(c + 1) * 256;
            r0 = nx[lane]; r1 = nx[64 + lane]; r2 = nx[128 + lane]; r3 = nx[192 + lane];
        }
        __syncthreads();
        if (lane == 0) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            f4 a0, a1, a2, a3, a4, a5, a6, a7, b0, b1, b2, b3, b4, b5, b6, b7;
            const uint32_t base = (uint32_t)(uintptr_t)buf;
#define YCGE_RD8(r0, r1, r2, r3, r4, r5, r6, r7, addr)                                                                                         \
            asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:16\n\tds_read_b128 %2, %8 offset:32\n\tds_read_b128 %3, %8 offset:48\n\t" \
                         "ds_read_b128 %4, %8 offset:64\n\tds_read_b128 %5, %8 offset:80\n\tds_read_b128 %6, %8 offset:96\n\tds_read_b128 %7, %8 offset:112" \
                         : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7) : "v"(addr) : "memory")
#define YCGE_WAIT8(n, r0, r1, r2, r3, r4, r5, r6, r7)                                                                                          \
            asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7))
#define YCGE_ADD8(r0, r1, r2, r3, r4, r5, r6, r7)                                                                                              \
            sum += r0.x; sum += r0.y; sum += r0.z; sum += r0.w; sum += r1.x; sum += r1.y; sum += r1.z; sum += r1.w; \
            sum += r2.x; sum += r2.y; sum += r2.z; sum += r2.w; sum += r3.x; sum += r3.y; sum += r3.z; sum += r3.w; \
            sum += r4.x; sum += r4.y; sum += r4.z; sum += r4.w; sum += r5.x; sum += r5.y; sum += r5.z; sum += r5.w; \
            sum += r6.x; sum += r6.y; sum += r6.z; sum += r6.w; sum += r7.x; sum += r7.y; sum += r7.z; sum += r7.w
            YCGE_RD8(a0, a1, a2, a3, a4, a5, a6, a7, base);
#pragma unroll 1
            for (uint32_t blk = 0; blk < 30; blk += 2) {        // 32 blocks of 8 float4 = the chunk's 1024 terms; no branch inside:
                YCGE_RD8(b0, b1, b2, b3, b4, b5, b6, b7, base + (blk + 1u) * 128u);     // the two sets must stay in their registers
                YCGE_WAIT8(8, a0, a1, a2, a3, a4, a5, a6, a7);
                YCGE_ADD8(a0, a1, a2, a3, a4, a5, a6, a7);
                YCGE_RD8(a0, a1, a2, a3, a4, a5, a6, a7, base + (blk + 2u) * 128u);
                YCGE_WAIT8(8, b0, b1, b2, b3, b4, b5, b6, b7);
                YCGE_ADD8(b0, b1, b2, b3, b4, b5, b6, b7);
            }
            YCGE_RD8(b0, b1, b2, b3, b4, b5, b6, b7, base + 31u * 128u);
            YCGE_WAIT8(8, a0, a1, a2, a3, a4, a5, a6, a7);
            YCGE_ADD8(a0, a1, a2, a3, a4, a5, a6, a7);
            YCGE_WAIT8(0, b0, b1, b2, b3, b4, b5, b6, b7);
            YCGE_ADD8(b0, b1, b2, b3, b4, b5, b6, b7);
#undef YCGE_RD8
#undef YCGE_WAIT8
#undef YCGE_ADD8
        }
        // the other buffer is written next; it was last read two iterations ago, before the barrier above
    }
    if (lane != 0) return;
    const float inv = 1.0f / (float)(int32_t)(uint32_t)(H->best >> 32);          // (float)triCount; at least one face: the parse refused the file otherwise
    H->sum[blockIdx.x] = sum;
    H->centroid[blockIdx.x] = __fmul_rn(sum, inv);
}

__global__ __launch_bounds__(kGroundBlock) void k_ground_bounds(const float *__restrict__ positions, uint32_t n_positions, const uint8_t *__restrict__ used, GroundHeader *H)
{
    const uint32_t v = blockIdx.x * (uint32_t)kGroundBlock + threadIdx.x;
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    const bool mine = v < n_positions && used[v] != 0;
    if (mine) {
        float p[3];
        for (int a = 0; a < 3; a++) p[a] = __fsub_rn(positions[3 * (size_t)v + a], H->centroid[a]);
        grow(lo, hi, p);
    }
    const unsigned long long m = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&H->n_used, (uint32_t)__popcll(m));
    reduce_box(lo, hi, H->box);
}

inline uint32_t blocks_of(uint32_t n, uint32_t per) { return (n + per - 1u) / per; }

} // namespace

// 0 bytes of the header the launchers share, 1 the terms one trip of the sum takes (each plane is padded to a multiple), 2 the round cap
extern "C" size_t ycge_launch_obj_ground_sizes(int which)
{
    return which == 0 ? sizeof(GroundHeader) : which == 1 ? (size_t)kGroundChunk : which == 2 ? (size_t)ycge_obj::kGroundRoundCap : 0;
}

// One labelling round: hook + flatten over parent (n_positions words).  first != 0: the header and parent are set up before it.
// header.changed: the round hooked something; header.decline.  Every index of faces is in range.
extern "C" int ycge_launch_obj_ground_round(const int32_t *faces, uint32_t n_triangles, uint32_t n_positions, uint32_t *parent, int first, void *header, hipStream_t stream)
{
    if (!faces || !parent || !header || n_triangles == 0 || n_positions == 0) return (int)hipErrorInvalidValue;
    GroundHeader *H = static_cast<GroundHeader *>(header);
    hipError_t e;
    if (first) {
        e = hipMemsetAsync(H, 0, sizeof(GroundHeader), stream);
        if (e == hipSuccess) e = hipMemsetAsync(&H->box[0], 0xff, 12, stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_ground_init, dim3(blocks_of(n_positions, kGroundBlock)), dim3(kGroundBlock), 0, stream, parent, n_positions);
    } else {
        e = hipMemsetAsync(&H->changed, 0, 4, stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k_ground_hook, dim3(blocks_of(n_triangles, kGroundBlock)), dim3(kGroundBlock), 0, stream, faces, n_triangles, n_positions, parent, H);
    hipLaunchKernelGGL(k_ground_flatten, dim3(blocks_of(n_positions, kGroundBlock)), dim3(kGroundBlock), 0, stream, parent, n_positions, H);
    return (int)hipGetLastError();
}

// the chosen component: count, first (n_positions words each, cleared here); header.best, n_components.  parent is flat.
extern "C" int ycge_launch_obj_ground_select(const int32_t *faces, uint32_t n_triangles, uint32_t n_positions, const uint32_t *parent, uint32_t *count, uint32_t *first,
                                             void *header, hipStream_t stream)
{
    if (!faces || !parent || !count || !first || !header || n_triangles == 0 || n_positions == 0) return (int)hipErrorInvalidValue;
    GroundHeader *H = static_cast<GroundHeader *>(header);
    hipError_t e = hipMemsetAsync(count, 0, (size_t)n_positions * 4, stream);
    if (e == hipSuccess) e = hipMemsetAsync(first, 0xff, (size_t)n_positions * 4, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_ground_count, dim3(blocks_of(n_triangles, kGroundBlock)), dim3(kGroundBlock), 0, stream, faces, n_triangles, parent, count, first);
    hipLaunchKernelGGL(k_ground_winner, dim3(blocks_of(n_positions, kGroundBlock)), dim3(kGroundBlock), 0, stream, (const uint32_t *)count, (const uint32_t *)first, n_positions, H);
    return (int)hipGetLastError();
}

// the terms (3 planes of `padded` floats, padded = n_triangles rounded up to the sum's trip) and used (n_positions bytes, cleared here)
extern "C" int ycge_launch_obj_ground_terms(const float *positions, const int32_t *faces, uint32_t n_triangles, uint32_t n_positions, const uint32_t *parent, float *terms,
                                            uint32_t padded, uint8_t *used, void *header, hipStream_t stream)
{
    if (!positions || !faces || !parent || !terms || !used || !header || n_triangles == 0 || n_positions == 0 || padded < n_triangles || padded % kGroundChunk != 0)
        return (int)hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(used, 0, n_positions, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_ground_terms, dim3(blocks_of(padded, kGroundBlock)), dim3(kGroundBlock), 0, stream, positions, faces, n_triangles, padded, parent,
                       (const GroundHeader *)header, terms, used);
    return (int)hipGetLastError();
}

// header.sum, header.centroid: one workgroup per axis
extern "C" int ycge_launch_obj_ground_sum(const float *terms, uint32_t padded, void *header, hipStream_t stream)
{
    if (!terms || !header || padded == 0 || padded % kGroundChunk != 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ground_sum, dim3(3), dim3(64), 0, stream, terms, padded, static_cast<GroundHeader *>(header));
    return (int)hipGetLastError();
}

// header.box, header.n_used
extern "C" int ycge_launch_obj_ground_bounds(const float *positions, uint32_t n_positions, const uint8_t *used, void *header, hipStream_t stream)
{
    if (!positions || !used || !header || n_positions == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ground_bounds, dim3(blocks_of(n_positions, kGroundBlock)), dim3(kGroundBlock), 0, stream, positions, n_positions, used, static_cast<GroundHeader *>(header));
    return (int)hipGetLastError();
}
