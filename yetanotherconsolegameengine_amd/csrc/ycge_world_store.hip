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
#include <hip/hip_runtime.h>

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

}  // namespace

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
