// ycge_worldgen.hip - WorldGenerator.GenerateChunkCells on the device (restatement: ycge_worldgen.h; host twin: ycge_worldgen.cpp).
//
// ycge_scene_generate_grids makes a batch of chunks where they will be traced: the raw (matId, metaId) cells are written straight into the
// area k_grid_encode (ycge_grid_encode.hip) reads, in ycge_grid.cells order.  Its own translation unit, as the other stages': the code
// objects of the frame kernels stay what they were.  Three kernels, all bound by VALU issue (integer hashing and fp32, about 40 octaves of
// gradient noise per HeightY), none with scratch:
//
// k_wg_columns   one workgroup of 256 lanes per DISTINCT (cx, cz) of the batch - every 2-D field is shared by the chunks stacked in a column.
//                HeightY once per cell of the (S + 2)^2 tile into LDS (ground and its 8 neighbours without re-evaluation), then, a barrier
//                between each: D8 direction; in-degree, carve; clamped slope on the carved heights, biome, LocalWaterY, lake override,
//                RockMetaAt's noise verdict -> one 16-byte record per column cell in global memory.  LDS is sized by the launch
//                ((S + 2)^2 + 2 S^2 words + S^2 bytes: 14 KB at S = 32, 54 KB at S = 64), so a chunk of 32 leaves room for four workgroups a CU;
//                the lanes' live state is small (a noise octave), occupancy is bounded by LDS and the 256-lane shape, not by registers.
// k_wg_fill      each lane owns PAIRS of consecutive cells of a chunk and writes them as one 16-byte store - consecutive lanes, consecutive
//                addresses - from the column records (L2-resident: 16 KB a chunk column at S = 32); any_solid is reduced per workgroup.
// k_wg_trees     one wavefront per chunk.  Trees only overwrite Air (or TallGrass), so the first tree in (lx, lz) order wins a cell, and
//                the no-leaves fallback crown depends on what earlier trees left: the wavefront finds its tree columns 64 at a time
//                (a ballot keeps them in (lx, lz) order) and places them SERIALLY in that order; one tree's trunk cells, then its canopy
//                cells, then the fallback crown are written in parallel, a barrier between the three.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_worldgen_host.h"

using namespace ycge;

namespace {

constexpr int kColBlock = 256, kFillBlock = 256, kFillPairsPerLane = 4;

__global__ __launch_bounds__(kColBlock) void k_wg_columns(const int32_t *__restrict__ col_keys, wg::World W, wg::ColRec *__restrict__ cols, int32_t *__restrict__ col_top)
{
    extern __shared__ int s_wg[];
    const int S = W.size, T2 = (S + 2) * (S + 2), S2 = S * S;
    int *tile = s_wg, *carved = tile + T2, *river_water = carved + S2;
    uint8_t *dir = (uint8_t *)(river_water + S2);
    __shared__ int s_top;
    const int t = (int)threadIdx.x;
    const int cx = col_keys[2 * blockIdx.x], cz = col_keys[2 * blockIdx.x + 1];
    const int base_x = cx * S, base_z = cz * S;
    if (t == 0) s_top = (int)0x80000000;
#pragma unroll 1
    for (int i = t; i < T2; i += kColBlock) {
        const int lx = i / (S + 2) - 1, lz = i % (S + 2) - 1;
        tile[i] = wg::height_y(base_x + lx, base_z + lz, W);
    }
    __syncthreads();
    for (int i = t; i < S2; i += kColBlock) dir[i] = (uint8_t)wg::d8_direction(tile, S, i / S, i % S);
    __syncthreads();
    for (int i = t; i < S2; i += kColBlock) {
        const int lx = i / S, lz = i % S;
        int rw;
        carved[i] = wg::river_carve(wg::river_accum(dir, S, lx, lz), wg::tile_at(tile, S, lx, lz), W.sea, &rw);
        river_water[i] = rw;
    }
    __syncthreads();
    int top = (int)0x80000000;
#pragma unroll 1
    for (int i = t; i < S2; i += kColBlock) {
        const int lx = i / S, lz = i % S;
        const wg::ColRec R = wg::column_record(carved, S, lx, lz, base_x + lx, base_z + lz, river_water[i], W);
        cols[(size_t)blockIdx.x * (size_t)S2 + (size_t)i] = R;
        const int m = R.ground > R.water ? R.ground : R.water;
        top = m > top ? m : top;
    }
    atomicMax(&s_top, top);
    __syncthreads();
    if (t == 0) col_top[blockIdx.x] = s_top;
}

__global__ __launch_bounds__(kFillBlock) void k_wg_fill(const WgChunk *__restrict__ chunks, wg::World W, const wg::ColRec *__restrict__ cols, uint32_t *__restrict__ any_solid)
{
    const WgChunk C = chunks[blockIdx.y];
    const int S = W.size, S2 = S * S, n_cells = S2 * S, n_pairs = (n_cells + 1) >> 1;
    const wg::ColRec *col = cols + (size_t)C.col * (size_t)S2;
    const int base_y = C.cy * S;
    int solid = 0;
    for (int p = (int)(blockIdx.x * kFillBlock + threadIdx.x); p < n_pairs; p += (int)(gridDim.x * kFillBlock)) {
        int v[4] = {0, 0, 0, 0};
        for (int k = 0; k < 2; k++) {
            const int i = 2 * p + k;
            if (i >= n_cells) break;
            const int lx = i / S2, rem = i - lx * S2, ly = rem / S, lz = rem - ly * S;
            wg::cell_at(col[lx * S + lz], base_y + ly, W, &v[2 * k], &v[2 * k + 1]);
            solid |= v[2 * k] != 0;
        }
        if (2 * p + 1 < n_cells) ((int4 *)C.cells)[p] = make_int4(v[0], v[1], v[2], v[3]);
        else ((int2 *)C.cells)[2 * p] = make_int2(v[0], v[1]);
    }
    if (__syncthreads_or(solid) && threadIdx.x == 0) atomicOr(&any_solid[blockIdx.y], 1u);
}

__global__ __launch_bounds__(64) void k_wg_trees(const WgChunk *__restrict__ chunks, wg::World W, const wg::ColRec *__restrict__ cols, uint32_t *__restrict__ any_solid)
{
    const WgChunk C = chunks[blockIdx.x];
    const int S = W.size, S2 = S * S;
    const wg::ColRec *col = cols + (size_t)C.col * (size_t)S2;
    const int base_x = C.cx * S, base_y = C.cy * S, base_z = C.cz * S;
    const int lane = (int)threadIdx.x;
    int2 *cells = (int2 *)C.cells;
    int solid = 0;
    for (int first = 0; first < S2; first += 64) {
        const int idx = first + lane;
        wg::Tree mine;
        mine.lx = mine.lz = mine.trunk_base = mine.trunk_h = mine.canopy_r = mine.canopy_base = mine.conifer = 0;
        bool has = false;
        if (idx < S2) {
            const int lx = idx / S, lz = idx - lx * S;
            has = wg::tree_at(col[idx], lx, lz, base_x + lx, base_z + lz, base_y, W, &mine);
        }
        unsigned long long todo = __ballot(has);
        while (todo) {          // (uniform: one wavefront) the tree columns of these 64, in (lx, lz) order
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            wg::Tree T;
            T.lx = __shfl(mine.lx, src); T.lz = __shfl(mine.lz, src); T.trunk_base = __shfl(mine.trunk_base, src); T.trunk_h = __shfl(mine.trunk_h, src);
            T.canopy_r = __shfl(mine.canopy_r, src); T.canopy_base = __shfl(mine.canopy_base, src); T.conifer = __shfl(mine.conifer, src);
            for (int k = lane; k < T.trunk_h; k += 64) {          // FloraPlacer.cs:72-81
                const int ly = T.trunk_base + k;
                if (ly < 0 || ly >= S) continue;
                const int cell = (T.lx * S + ly) * S + T.lz;
                if (wg::tree_may_replace(cells[cell].x)) { cells[cell] = make_int2(wg::kWood, 0); solid = 1; }
            }
            __syncthreads();
            const int dy_min = wg::tree_dy_min(T), n_canopy = (3 - dy_min) * 49;          // :84-109 over (dy, rx, rz) in a 7 x 7 window (canopyR <= 3)
            int leaves = 0;
            for (int k = lane; k < n_canopy; k += 64) {
                const int dy = dy_min + k / 49, r = k % 49, rx = r / 7 - 3, rz = r % 7 - 3;
                const int radius = wg::tree_radius(T, dy);
                if (rx < -radius || rx > radius || rz < -radius || rz > radius) continue;
                const int ly = T.canopy_base + dy, lx2 = T.lx + rx, lz2 = T.lz + rz;
                if (ly < 0 || ly >= S || lx2 < 0 || lx2 >= S || lz2 < 0 || lz2 >= S) continue;
                const int cell = (lx2 * S + ly) * S + lz2;
                if (wg::tree_may_replace(cells[cell].x)) { cells[cell] = make_int2(wg::kLeaves, 0); solid = 1; leaves = 1; }
            }
            if (!__syncthreads_or(leaves)) {          // :112-131
                const int ly = T.trunk_base + T.trunk_h - 1;
                if (ly >= 0 && ly < S && lane < 9) {
                    const int lx2 = T.lx + lane / 3 - 1, lz2 = T.lz + lane % 3 - 1;
                    if (lx2 >= 0 && lx2 < S && lz2 >= 0 && lz2 < S) {
                        const int cell = (lx2 * S + ly) * S + lz2;
                        if (cells[cell].x == wg::kAir) { cells[cell] = make_int2(wg::kLeaves, 0); solid = 1; }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (__syncthreads_or(solid) && lane == 0) atomicOr(&any_solid[blockIdx.x], 1u);
}

}  // namespace

extern "C" int ycge_launch_worldgen_columns(const int32_t *col_keys, int n_cols, const wg::World *W, wg::ColRec *cols, int32_t *col_top, void *stream)
{
    if (n_cols <= 0) return 0;
    const int S = W->size;
    const size_t lds = ((size_t)(S + 2) * (S + 2) + 2 * (size_t)S * S) * sizeof(int) + (((size_t)S * S + 3) & ~(size_t)3);
    hipLaunchKernelGGL(k_wg_columns, dim3((unsigned)n_cols), dim3(kColBlock), lds, (hipStream_t)stream, col_keys, *W, cols, col_top);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_worldgen_fill(const WgChunk *chunks, int n_chunks, const wg::World *W, const wg::ColRec *cols, uint32_t *any_solid, void *stream)
{
    if (n_chunks <= 0) return 0;
    const int S = W->size, n_pairs = (S * S * S + 1) / 2;
    const int per_block = kFillBlock * kFillPairsPerLane;
    const unsigned bx = (unsigned)((n_pairs + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_wg_fill, dim3(bx, (unsigned)n_chunks), dim3(kFillBlock), 0, (hipStream_t)stream, chunks, *W, cols, any_solid);
    int e = (int)hipGetLastError();
    if (e != 0) return e;
    hipLaunchKernelGGL(k_wg_trees, dim3((unsigned)n_chunks), dim3(64), 0, (hipStream_t)stream, chunks, *W, cols, any_solid);
    return (int)hipGetLastError();
}
