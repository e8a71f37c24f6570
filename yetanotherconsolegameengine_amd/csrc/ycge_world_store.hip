// ycge_world_store.hip - the kernels over a VG01 world that is resident on the device (ycge_world_store.cpp): AttachChunkFromPreloaded's two loops
// (WorldManager.cs:696-720), the any-cell-not-Air test per chunk and the slice of a chunk out of the world.  Both are copies or reads of 8-byte cells
// with no arithmetic: memory-bound, one cell (8 bytes) a lane, consecutive lanes on consecutive cells along z - the world's fastest axis - so a
// wavefront's access is whole rows of its chunk.  No LDS, no scratch (profiles/world_store_resources.txt).
//   k_ws_occupied   one wavefront per (x-plane, cy, cz): the sy x sz cells the chunk has in that plane.  Each lane ORs mat != 0 over its cells, a
//                   ballot makes the wavefront's flag, lane 0 ORs it into the chunk's word - one vector atomic a wavefront, and none when the
//                   plane holds nothing of the chunk.  A plane belongs to one slab of the load, so slab borders may fall anywhere; the words
//                   collect over the slabs.  A wavefront whose chunk's word is set already (an earlier plane's, or slab's) reads no cell.
//   k_ws_slice      blockIdx.y = chunk of the group: cell i of the destination (ycge_grid.cells order) from the store, by the chunk's record.
//                   The 8-byte form only: with an odd nz or an odd clipped sz no row pair starts 16-byte aligned, and the aligned worlds gain
//                   nothing that has been measured.
//   k_ws_edit       ycge_world_store_edit: one lane per cell of an op's box writes the op's pair (described at the kernel).
//   k_ws_pool_*     the pool of materialised chunks beside a fields store: edit, occupancy, copy into an attach, planes into a read's slab
//                   (described at the kernels; profiles/world_store_pool_resources.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ycge_world_store.h"

using namespace ycge;

namespace {

constexpr int kBlock = 256, kWave = 64, kSliceCellsPerLane = 4;

__global__ __launch_bounds__(kBlock) void k_ws_occupied(const int2 *__restrict__ cells, WsShape W, int x0, int planes, uint32_t *__restrict__ occupied)
{
    const uint32_t per_plane = (uint32_t)W.ncy * (uint32_t)W.ncz;
    const uint64_t w = (uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;          // (wavefront-uniform)
    if (w >= (uint64_t)planes * per_plane) return;
    const int x = x0 + (int)(w / per_plane), cy = (int)((w % per_plane) / (uint32_t)W.ncz), cz = (int)(w % (uint32_t)W.ncz);
    uint32_t *word = occupied + ((size_t)(x / W.S) * W.ncy + cy) * W.ncz + cz;
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;          // (a stale 0 costs the reads only)
    const int sy = min(W.S, W.ny - cy * W.S), sz = min(W.S, W.nz - cz * W.S);
    const int2 *plane = cells + ((size_t)x * W.ny + (size_t)cy * W.S) * W.nz + (size_t)cz * W.S;
    const int n = sy * sz, lane = threadIdx.x % kWave;
    for (int first = 0; first < n; first += 4 * kWave) {
        int found = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = first + u * kWave + lane;
            if (t < n) found |= plane[(size_t)(t / sz) * W.nz + t % sz].x != 0;
        }
        if (__ballot(found) != 0ull) {
            if (lane == 0) atomicOr(word, 1u);
            return;
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_ws_slice(const int2 *__restrict__ cells, WsShape W, const WsChunk *__restrict__ chunks)
{
    const WsChunk C = chunks[blockIdx.y];
    const uint32_t n = (uint32_t)C.sx * (uint32_t)C.sy * (uint32_t)C.sz, plane = (uint32_t)C.sy * (uint32_t)C.sz;          // (< 2^30: S <= 1024)
    const int2 *src = cells + C.src;
    int2 *dst = (int2 *)C.dst;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t lx = i / plane, r = i % plane, ly = r / (uint32_t)C.sz, lz = r % (uint32_t)C.sz;
        dst[i] = src[((size_t)lx * W.ny + ly) * W.nz + lz];
    }
}

// ycge_world_store_edit.  blockIdx.y = op j of the launch, one lane per cell of its box (grid-stride).  The ops of a launch may overlap and the
// later op wins: a lane walks the ops AFTER its own in list order and leaves its cell alone when one of them covers it - that op's lane
// writes it - so every cell is written by exactly one lane, that of the last op that covers it, whatever order the workgroups run in.
// The walk reads the ops at workgroup-uniform addresses (scalar loads) and skips an op whose box misses op j's by a uniform branch.
// Launches follow each other on one stream, so the rule holds across them.  Plain 8-byte vector stores, no atomics, no LDS, no scratch.
__global__ __launch_bounds__(kBlock) void k_ws_edit(int2 *__restrict__ cells, WsShape W, const WsEditOp *__restrict__ ops, int m)
{
    const int j = (int)blockIdx.y;
    const WsEditOp E = ops[j];
    const uint32_t sy = (uint32_t)(E.hi[1] - E.lo[1] + 1), sz = (uint32_t)(E.hi[2] - E.lo[2] + 1);
    const uint64_t plane = (uint64_t)sy * sz, n = (uint64_t)(uint32_t)(E.hi[0] - E.lo[0] + 1) * plane;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        const int x = E.lo[0] + (int)(i / plane);
        const uint32_t r = (uint32_t)(i % plane);
        const int y = E.lo[1] + (int)(r / sz), z = E.lo[2] + (int)(r % sz);
        bool later = false;
        for (int k = j + 1; k < m; k++) {
            const WsEditOp L = ops[k];
            if (L.hi[0] < E.lo[0] || L.lo[0] > E.hi[0] || L.hi[1] < E.lo[1] || L.lo[1] > E.hi[1] || L.hi[2] < E.lo[2] || L.lo[2] > E.hi[2]) continue;          // (uniform)
            later |= x >= L.lo[0] && x <= L.hi[0] && y >= L.lo[1] && y <= L.hi[1] && z >= L.lo[2] && z <= L.hi[2];
        }
        if (!later) cells[((size_t)x * W.ny + (size_t)y) * W.nz + (size_t)z] = make_int2(E.mat, E.meta);
    }
}

// ---- the pool of materialised chunks beside a fields store (ycge_world_store_reserve_edits).  A slot is a chunk's S^3 cells in
// ycge_grid.cells order (z fastest), so a lane per cell along z reads or writes whole rows of the slot.  S^3 < 2^31 (k_wp_fill's own limit).
inline __device__ int2 *slot_cells(uint8_t *pool, size_t stride, int slot) { return (int2 *)(pool + (size_t)slot * stride); }
inline __device__ const int2 *slot_cells(const uint8_t *pool, size_t stride, int slot) { return (const int2 *)(pool + (size_t)slot * stride); }

// ycge_world_store_edit on a pooled fields store.  blockIdx.y = record j of the launch - an op clipped against one chunk - one lane per
// cell of its box, lanes along z (grid-stride).  k_ws_edit's rule, slot by slot: the records are sorted by slot with list order inside a
// slot, and a lane walks the records AFTER its own while they name its slot and leaves its cell alone when one of them covers it - that
// record's lane writes it.  So every cell is written by exactly one lane, that of the last op that covers it.  The walk reads the records
// at workgroup-uniform addresses and ends at the first record of another slot.  Launches follow each other on one stream, so the rule
// holds across them.  Plain 8-byte vector stores, no atomics, no LDS, no scratch.
__global__ __launch_bounds__(kBlock) void k_ws_pool_edit(uint8_t *__restrict__ pool, size_t stride, int S, const WsPoolEdit *__restrict__ recs, int m)
{
    const int j = (int)blockIdx.y;
    const WsPoolEdit E = recs[j];
    const uint32_t sy = (uint32_t)(E.hi[1] - E.lo[1] + 1), sz = (uint32_t)(E.hi[2] - E.lo[2] + 1);
    const uint32_t plane = sy * sz, n = (uint32_t)(E.hi[0] - E.lo[0] + 1) * plane;
    int2 *cells = slot_cells(pool, stride, E.slot);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t r = i % plane;
        const int x = E.lo[0] + (int)(i / plane), y = E.lo[1] + (int)(r / sz), z = E.lo[2] + (int)(r % sz);
        bool later = false;
        for (int k = j + 1; k < m; k++) {
            const WsPoolEdit L = recs[k];
            if (L.slot != E.slot) break;          // (uniform, as the next)
            if (L.hi[0] < E.lo[0] || L.lo[0] > E.hi[0] || L.hi[1] < E.lo[1] || L.lo[1] > E.hi[1] || L.hi[2] < E.lo[2] || L.lo[2] > E.hi[2]) continue;
            later |= x >= L.lo[0] && x <= L.hi[0] && y >= L.lo[1] && y <= L.hi[1] && z >= L.lo[2] && z <= L.hi[2];
        }
        if (!later) cells[((size_t)x * S + (size_t)y) * S + (size_t)z] = make_int2(E.mat, E.meta);
    }
}

// blockIdx.y = slot j of the list; a wavefront takes 4 * kWave consecutive cells of it.  Each lane ORs mat != 0 over its four cells, one
// ballot makes the wavefront's flag and lane 0 ORs it into the slot's word: at most one vector atomic a wavefront, as k_ws_occupied.  A
// wavefront whose slot's word is set already reads no cell.
__global__ __launch_bounds__(kBlock) void k_ws_pool_occupied(const uint8_t *__restrict__ pool, size_t stride, int S, const int32_t *__restrict__ slots, uint32_t *__restrict__ words)
{
    const uint32_t n = (uint32_t)S * (uint32_t)S * (uint32_t)S;
    const uint64_t first = ((uint64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave) * (4 * kWave);          // (wavefront-uniform)
    if (first >= n) return;
    uint32_t *word = words + blockIdx.y;
    if (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return;          // (a stale 0 costs the reads only)
    const int2 *cells = slot_cells(pool, stride, slots[blockIdx.y]);
    const uint32_t lane = threadIdx.x % kWave;
    int found = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint64_t t = first + (uint32_t)u * kWave + lane;
        if (t < n) found |= cells[t].x != 0;
    }
    if (__ballot(found) != 0ull && lane == 0) atomicOr(word, 1u);
}

// blockIdx.y = record j: a whole slot into the cells of a grid of an attach, two cells (16 bytes) a lane as k_wp_fill writes them; an odd S^3 ends in one 8-byte cell
__global__ __launch_bounds__(kBlock) void k_ws_pool_copy(const uint8_t *__restrict__ pool, size_t stride, int S, const WsPoolCopy *__restrict__ recs)
{
    const WsPoolCopy C = recs[blockIdx.y];
    const uint32_t n = (uint32_t)S * (uint32_t)S * (uint32_t)S, n_pairs = (n + 1) >> 1;
    const int2 *src = slot_cells(pool, stride, C.slot);
    for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n_pairs; p += gridDim.x * kBlock) {
        if (2 * p + 1 < n) ((int4 *)C.dst)[p] = ((const int4 *)src)[p];
        else ((int2 *)C.dst)[2 * p] = src[2 * p];
    }
}

// ycge_world_store_read on a pooled fields store, behind k_wp_planes: blockIdx.y = record j, the R.n x-planes of a slot that lie in the
// slab; one lane per cell, lanes along z, so a wavefront reads consecutive cells of the slot and writes pieces of rows of the slab.
__global__ __launch_bounds__(kBlock) void k_ws_pool_planes(const uint8_t *__restrict__ pool, size_t stride, int S, const WsPoolPlanes *__restrict__ recs, int2 *__restrict__ slab, int ny, int nz)
{
    const WsPoolPlanes R = recs[blockIdx.y];
    const uint32_t plane = (uint32_t)S * (uint32_t)S, n = (uint32_t)R.n * plane;
    const int2 *src = slot_cells(pool, stride, R.slot) + (size_t)R.lx0 * plane;
    int2 *dst = slab + ((size_t)R.px * (size_t)ny + (size_t)R.cy * (size_t)S) * (size_t)nz + (size_t)R.cz * (size_t)S;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const uint32_t lx = i / plane, r = i % plane, ly = r / (uint32_t)S, lz = r % (uint32_t)S;
        dst[((size_t)lx * (size_t)ny + ly) * (size_t)nz + lz] = src[i];
    }
}

}  // namespace

extern "C" int ycge_launch_world_store_edit(int32_t *cells, const WsShape *shape, const WsEditOp *ops, int m, uint64_t max_cells, void *stream)
{
    if (m <= 0 || max_cells == 0) return 0;
    if (m > YCGE_WS_EDIT_OPS_PER_LAUNCH) return (int)hipErrorInvalidValue;
    const uint64_t per_block = (uint64_t)kBlock * kSliceCellsPerLane;
    const uint64_t bx = std::min<uint64_t>((max_cells + per_block - 1) / per_block, 65536);
    hipLaunchKernelGGL(k_ws_edit, dim3((unsigned)bx, (unsigned)m), dim3(kBlock), 0, (hipStream_t)stream, (int2 *)cells, *shape, ops, m);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_world_store_occupied(const int32_t *cells, const WsShape *shape, int32_t x0, int32_t planes, uint32_t *occupied, void *stream)
{
    const uint64_t waves = (uint64_t)planes * (uint64_t)shape->ncy * (uint64_t)shape->ncz, blocks = (waves + kBlock / kWave - 1) / (kBlock / kWave);
    if (x0 < 0 || planes <= 0 || x0 + planes > shape->nx || blocks == 0 || blocks > 0x7fffffffull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ws_occupied, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, (const int2 *)cells, *shape, x0, planes, occupied);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_world_store_slice(const int32_t *cells, const WsShape *shape, const WsChunk *chunks, int m, size_t max_cells, void *stream)
{
    if (m <= 0 || max_cells == 0) return 0;
    if (m > 65535) return (int)hipErrorInvalidValue;
    const size_t per_block = (size_t)kBlock * kSliceCellsPerLane;
    const unsigned bx = (unsigned)((max_cells + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_ws_slice, dim3(bx, (unsigned)m), dim3(kBlock), 0, (hipStream_t)stream, (const int2 *)cells, *shape, chunks);
    return (int)hipGetLastError();
}

namespace {
// blocks along x for a launch whose largest record holds n lanes' worth of work, kSliceCellsPerLane a lane
inline unsigned pool_blocks(uint64_t n)
{
    const uint64_t per_block = (uint64_t)kBlock * kSliceCellsPerLane;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, 65536));
}
inline bool pool_args_bad(const void *pool, size_t stride, int S, const void *recs, int m)
{
    return !pool || !recs || m > 65535 || S < 1 || (uint64_t)S * S * S >= (1ull << 31) || stride % 16 != 0 || stride < (uint64_t)S * S * S * 8;
}
}  // namespace

extern "C" int ycge_launch_world_store_pool_edit(uint8_t *pool, size_t stride, int S, const WsPoolEdit *recs, int m, uint64_t max_cells, void *stream)
{
    if (m <= 0 || max_cells == 0) return 0;
    if (pool_args_bad(pool, stride, S, recs, m)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ws_pool_edit, dim3(pool_blocks(max_cells), (unsigned)m), dim3(kBlock), 0, (hipStream_t)stream, pool, stride, S, recs, m);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_world_store_pool_occupied(const uint8_t *pool, size_t stride, int S, const int32_t *slots, int m, uint32_t *words, void *stream)
{
    if (m <= 0) return 0;
    if (pool_args_bad(pool, stride, S, slots, m) || !words) return (int)hipErrorInvalidValue;
    const uint64_t n = (uint64_t)S * S * S, per_block = (uint64_t)(kBlock / kWave) * 4 * kWave;
    hipLaunchKernelGGL(k_ws_pool_occupied, dim3((unsigned)((n + per_block - 1) / per_block), (unsigned)m), dim3(kBlock), 0, (hipStream_t)stream, pool, stride, S, slots, words);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_world_store_pool_copy(const uint8_t *pool, size_t stride, int S, const WsPoolCopy *recs, int m, void *stream)
{
    if (m <= 0) return 0;
    if (pool_args_bad(pool, stride, S, recs, m)) return (int)hipErrorInvalidValue;
    const uint64_t n_pairs = ((uint64_t)S * S * S + 1) / 2;
    hipLaunchKernelGGL(k_ws_pool_copy, dim3(pool_blocks(n_pairs), (unsigned)m), dim3(kBlock), 0, (hipStream_t)stream, pool, stride, S, recs);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_world_store_pool_planes(const uint8_t *pool, size_t stride, int S, const WsPoolPlanes *recs, int m, int32_t *slab, int32_t ny, int32_t nz, void *stream)
{
    if (m <= 0) return 0;
    if (pool_args_bad(pool, stride, S, recs, m) || !slab || ny < S || nz < S) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ws_pool_planes, dim3(pool_blocks((uint64_t)S * S * S), (unsigned)m), dim3(kBlock), 0, (hipStream_t)stream, pool, stride, S, recs, (int2 *)slab, (int)ny, (int)nz);
    return (int)hipGetLastError();
}
