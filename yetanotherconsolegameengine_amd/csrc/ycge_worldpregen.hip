// ycge_worldpregen.hip - WorldManager.GenerateAndSaveWorld on the device (restatement: the second half of ycge_worldgen.h; host twin:
// ycge_worldgen.cpp).  ycge_scene_generate_world makes the reference's pregenerated world where it will be traced; no 3-D array of the
// world exists on the device, only 2-D fields of the window (about 40 bytes a column) and the sub-batch of chunks being encoded.
//
// 2-D stages, one lane per column of the window, each a launch of its own because each reads its predecessor's NEIGHBOURS:
//   k_wp_height      TerrainNoise.HeightY (all the noise: VALU bound, about 40 octaves a column)
//   k_wp_d8          RiverNetworkGlobal's D8 direction
//   k_wp_carve       the in-degree count (see wg::river_accum_global), carve depth, river surface
//   k_wp_columns     slope on the carved ground, biome, LocalWaterY, the lake override, RockMetaAt's verdict -> the 16-byte column record;
//                    the feature descriptor (a pure function of the record); the fallback flag zeroed
//   k_wp_reach       the highest y any feature rooted within 3 columns may write: above it a cell is its base cell and the fill scans nothing
// FloraPlacer.PlaceTreesGlobal is serial, but every write turns a cell non-Air and no feature replaces anything else, so a cell belongs to
// the FIRST feature in the serial order whose write set covers it: a gather over the 7 x 7 columns around the cell (wg::world_cell), no
// atomics.  The one thing a tree's write set depends on is anyLeaves (its fallback crown), which depends on the features before it:
//   k_wp_any_leaves  one lane per column, working where a tree stands: anyLeaves by the same gather from the CURRENT flags into the next
//                    flags, counting the flips; the host repeats it until a pass flips nothing (the dependence is strictly backward in the
//                    serial order, so after pass k the first k trees are final)
//   k_wp_occupied    one word per chunk: does the finished chunk hold a cell that is not Air (AttachChunkFromPreloaded's anySolid)?  A lane
//                    marks its column's chunks up to max(ground, localWater) and, above, the chunk of every feature cell the gather finds -
//                    exact chunk by chunk: a small chunk between the ground and a neighbouring tree's canopy can be all Air
//   k_wp_fill        as k_wg_fill: each lane owns pairs of consecutive cells of a chunk and writes them as one 16-byte store into the area
//                    k_grid_encode reads; the cell is the base cell, or, at or below the column's reach, the gather
//   k_wp_planes      the same cells as whole x-planes in VG01 order, one lane per column walking a run of y: the payload of a world file, slab by
//                    slab (ycge_world_store_read on a fields store), or a device cell store (ycge_world_store_generate, CELLS form).  No LDS,
//                    no atomics, no scratch (profiles/world_store_generate_resources.txt)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_worldgen_host.h"

using namespace ycge;

namespace {

constexpr int kBlock = 256, kFillPairsPerLane = 4;

__global__ __launch_bounds__(kBlock) void k_wp_height(wg::World W, wg::Window N, int32_t *__restrict__ ground0)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    ground0[i] = wg::height_y(N.ox + i / N.nz, N.oz + i % N.nz, W);
}

__global__ __launch_bounds__(kBlock) void k_wp_d8(wg::Window N, const int32_t *__restrict__ ground0, uint8_t *__restrict__ dir)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    dir[i] = (uint8_t)wg::d8_global(ground0, N.nx, N.nz, i / N.nz, i % N.nz);
}

__global__ __launch_bounds__(kBlock) void k_wp_carve(wg::World W, wg::Window N, const int32_t *__restrict__ ground0, const uint8_t *__restrict__ dir,
                                                     int32_t *__restrict__ ground, int32_t *__restrict__ river_water)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    int rw;
    ground[i] = wg::river_carve(wg::river_accum_global(dir, N.nx, N.nz, i / N.nz, i % N.nz), ground0[i], W.sea, &rw);
    river_water[i] = rw;
}

__global__ __launch_bounds__(kBlock) void k_wp_columns(wg::World W, wg::Window N, const int32_t *__restrict__ ground, const int32_t *__restrict__ river_water,
                                                       wg::ColRec *__restrict__ rec, uint32_t *__restrict__ feat, uint8_t *__restrict__ fallback)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    const int x = i / N.nz, z = i % N.nz;
    const wg::ColRec R = wg::column_record_global(ground, N, x, z, river_water[i], W);
    rec[i] = R;
    feat[i] = wg::feature_at(R, N.ox + x, N.oz + z, W);
    fallback[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_wp_reach(wg::Window N, const wg::ColRec *__restrict__ rec, const uint32_t *__restrict__ feat, int32_t *__restrict__ reach)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    const int x = i / N.nz, z = i % N.nz;
    const int fx0 = max(x - wg::kFeatReach, 0), fx1 = min(x + wg::kFeatReach, N.nx - 1), fz0 = max(z - wg::kFeatReach, 0), fz1 = min(z + wg::kFeatReach, N.nz - 1);
    int hi = -1;
    for (int fx = fx0; fx <= fx1; fx++)
        for (int fz = fz0; fz <= fz1; fz++) {
            const uint32_t d = feat[fx * N.nz + fz];
            if (d != wg::kFeatNone) hi = max(hi, wg::feat_top(d, rec[fx * N.nz + fz].ground));
        }
    reach[i] = hi;
}

__global__ __launch_bounds__(kBlock) void k_wp_any_leaves(wg::World W, wg::Window N, const wg::ColRec *__restrict__ rec, const uint32_t *__restrict__ feat,
                                                          const uint8_t *__restrict__ fallback, uint8_t *__restrict__ next, uint32_t *__restrict__ changed)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    uint8_t f = 0;
    if (wg::feat_kind(feat[i]) == wg::kFeatTree) f = wg::tree_any_leaves(rec, feat, fallback, N, W, i / N.nz, i % N.nz) ? 0 : 1;
    next[i] = f;
    if (f != fallback[i]) atomicAdd(changed, 1u);          // (rare: a tree whose whole canopy was taken)
}

__global__ __launch_bounds__(kBlock) void k_wp_occupied(wg::World W, wg::Window N, int chunks_y, int chunks_z, const wg::ColRec *__restrict__ rec,
                                                        const uint32_t *__restrict__ feat, const uint8_t *__restrict__ fallback, const int32_t *__restrict__ reach,
                                                        uint32_t *__restrict__ occupied)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= N.nx * N.nz) return;
    const int x = i / N.nz, z = i % N.nz, S = W.size;
    const wg::ColRec R = rec[i];
    uint32_t *col = occupied + (size_t)(x / S) * (size_t)chunks_y * (size_t)chunks_z + (size_t)(z / S);          // chunk cy of this column: col[cy * chunks_z]
    const int base_top = min(max(R.ground, R.water), W.height - 1);          // solid up to the ground, Water up to localWater: no Air at or below
    for (int cy = base_top / S; cy >= 0; cy--) col[(size_t)cy * chunks_z] = 1u;          // (every lane that marks a chunk stores the same word)
    // above: Air but for the features' cells, and a chunk between the ground and a neighbour's canopy may hold none - cell by cell
    for (int y = base_top + 1, hi = min(reach[i], W.height - 1); y <= hi; y++) {
        int mat, meta;
        wg::world_cell(rec, feat, fallback, N, W, x, y, z, &mat, &meta);
        if (mat != wg::kAir) col[(size_t)(y / S) * chunks_z] = 1u;
    }
}

__global__ __launch_bounds__(kBlock) void k_wp_fill(const WgChunk *__restrict__ chunks, wg::World W, wg::Window N, const wg::ColRec *__restrict__ rec,
                                                    const uint32_t *__restrict__ feat, const uint8_t *__restrict__ fallback, const int32_t *__restrict__ reach,
                                                    uint32_t *__restrict__ any_solid)
{
    const WgChunk C = chunks[blockIdx.y];
    const int S = W.size, S2 = S * S, n_cells = S2 * S, n_pairs = (n_cells + 1) >> 1;
    const int base_x = C.cx * S, base_y = C.cy * S, base_z = C.cz * S;
    int solid = 0;
    for (int p = (int)(blockIdx.x * kBlock + threadIdx.x); p < n_pairs; p += (int)(gridDim.x * kBlock)) {
        int v[4] = {0, 0, 0, 0};
        for (int k = 0; k < 2; k++) {
            const int i = 2 * p + k;
            if (i >= n_cells) break;
            const int lx = i / S2, rem = i - lx * S2, ly = rem / S, lz = rem - ly * S;
            const int x = base_x + lx, y = base_y + ly, z = base_z + lz, col = x * N.nz + z;
            if (y > reach[col]) wg::cell_at_global(rec[col], y, W, &v[2 * k], &v[2 * k + 1]);
            else wg::world_cell(rec, feat, fallback, N, W, x, y, z, &v[2 * k], &v[2 * k + 1]);
            solid |= v[2 * k] != 0;
        }
        if (2 * p + 1 < n_cells) ((int4 *)C.cells)[p] = make_int4(v[0], v[1], v[2], v[3]);
        else ((int2 *)C.cells)[2 * p] = make_int2(v[0], v[1]);
    }
    if (__syncthreads_or(solid) && threadIdx.x == 0) atomicOr(&any_solid[blockIdx.y], 1u);
}

// Whole x-planes of the finished world in VG01 order (x, then y, then z fastest).  One lane per column (x, z) and run of y_seg cells along
// y (blockIdx.y), consecutive lanes along z: the lane loads its record and reach once and walks its run, and per y a wavefront stores one
// contiguous run of 64 cells (512 bytes) of the row (x, y, .).  The runs along y are there for the lanes' number alone: a slab of 64 MiB
// of the reference's world is 32 planes of 1024 columns, half a wavefront per SIMD when a lane walks the whole column (the 32 slabs of
// the 2 GiB world, each followed by k_ws_occupied: 15.4 ms that way, 9.6 ms with runs of 16 - NOTEBOOK.md).  8-byte stores: nz is odd whenever S and chunks_z
// are, and then no row pair starts 16-byte aligned.  blockIdx.x counts (plane, block of kBlock columns along z).  `cells`: the first
// cell of plane x0.
__global__ __launch_bounds__(kBlock) void k_wp_planes(wg::World W, wg::Window N, int x0, int z_blocks, int y_seg, const wg::ColRec *__restrict__ rec,
                                                      const uint32_t *__restrict__ feat, const uint8_t *__restrict__ fallback, const int32_t *__restrict__ reach,
                                                      int2 *__restrict__ cells)
{
    const int px = (int)(blockIdx.x / (unsigned)z_blocks), z = (int)(blockIdx.x % (unsigned)z_blocks) * kBlock + (int)threadIdx.x;
    if (z >= N.nz) return;
    const int x = x0 + px, col = x * N.nz + z, ny = W.height;
    const int y_begin = (int)blockIdx.y * y_seg, y_end = min(ny, y_begin + y_seg);
    const wg::ColRec R = rec[col];
    const int hi = reach[col];
    int2 *out = cells + (size_t)px * (size_t)ny * (size_t)N.nz + (size_t)z;
    for (int y = y_begin; y < y_end; y++) {
        int mat, meta;
        if (y > hi) wg::cell_at_global(R, y, W, &mat, &meta);
        else wg::world_cell(rec, feat, fallback, N, W, x, y, z, &mat, &meta);
        out[(size_t)y * (size_t)N.nz] = make_int2(mat, meta);
    }
}

inline unsigned blocks_for(const wg::Window *N) { return (unsigned)(((size_t)N->nx * N->nz + kBlock - 1) / kBlock); }

}  // namespace

extern "C" int ycge_launch_worldpregen_fields(const wg::World *W, const wg::Window *N, const WpFields *F, void *stream)
{
    const dim3 g(blocks_for(N)), b(kBlock);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_wp_height, g, b, 0, s, *W, *N, F->ground0);
    hipLaunchKernelGGL(k_wp_d8, g, b, 0, s, *N, F->ground0, F->dir);
    hipLaunchKernelGGL(k_wp_carve, g, b, 0, s, *W, *N, F->ground0, F->dir, F->ground, F->river_water);
    hipLaunchKernelGGL(k_wp_columns, g, b, 0, s, *W, *N, F->ground, F->river_water, F->rec, F->feat, F->fallback);
    hipLaunchKernelGGL(k_wp_reach, g, b, 0, s, *N, F->rec, F->feat, F->reach);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_worldpregen_any_leaves(const wg::World *W, const wg::Window *N, const WpFields *F, uint8_t *next, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(F->changed, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_wp_any_leaves, dim3(blocks_for(N)), dim3(kBlock), 0, s, *W, *N, F->rec, F->feat, F->fallback, next, F->changed);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_worldpregen_occupied(const wg::World *W, const wg::Window *N, const WpFields *F, int chunks_y, int chunks_z, size_t n_chunks, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(F->occupied, 0, n_chunks * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_wp_occupied, dim3(blocks_for(N)), dim3(kBlock), 0, s, *W, *N, chunks_y, chunks_z, F->rec, F->feat, F->fallback, F->reach, F->occupied);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_worldpregen_planes(const wg::World *W, const wg::Window *N, const WpFields *F, int32_t x0, int32_t planes, int32_t *cells, void *stream)
{
    const uint64_t z_blocks = ((uint64_t)N->nz + kBlock - 1) / kBlock, blocks = (uint64_t)(planes > 0 ? planes : 0) * z_blocks;
    const int y_seg = W->height <= 16 * 65535 ? 16 : 32;          // (gridDim.y; the height is 2^20 at most)
    const unsigned y_segs = (unsigned)((W->height + y_seg - 1) / y_seg);
    if (x0 < 0 || planes <= 0 || (int64_t)x0 + planes > N->nx || !cells || blocks > 0x7fffffffull || y_segs == 0 || y_segs > 65535u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_wp_planes, dim3((unsigned)blocks, y_segs), dim3(kBlock), 0, (hipStream_t)stream, *W, *N, x0, (int)z_blocks, y_seg, F->rec, F->feat, F->fallback, F->reach,
                       (int2 *)cells);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_worldpregen_fill(const WgChunk *chunks, int n_chunks, const wg::World *W, const wg::Window *N, const WpFields *F, uint32_t *any_solid, void *stream)
{
    if (n_chunks <= 0) return 0;
    const int S = W->size, n_pairs = (S * S * S + 1) / 2;
    const int per_block = kBlock * kFillPairsPerLane;
    const unsigned bx = (unsigned)((n_pairs + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_wp_fill, dim3(bx, (unsigned)n_chunks), dim3(kBlock), 0, (hipStream_t)stream, chunks, *W, *N, F->rec, F->feat, F->fallback, F->reach, any_solid);
    return (int)hipGetLastError();
}
