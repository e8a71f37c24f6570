// ycge_grid_encode.hip - the VolumeGrid ctor's per-voxel work on the device (host side: ycge_grid_encode.cpp).
//
// ycge_scene_attach_grids brings the raw cells of a batch of grids up once - 8 bytes a voxel, (matId, metaId), z fastest - and this
// kernel writes what the host loop of ycge_scene_upload writes: one byte a voxel at brick * 512 + morton3(x & 7, y & 7, z & 7), bricks
// padded to 8^3 with zeros; the index box of the solid voxels; the brick mask; the lowest cell that has no material.  Its own
// translation unit, as ycge_query.hip and ycge_chexel.hip are: the code objects of the frame kernels stay what they were.
//
// A workgroup of 256 lanes takes a run of YCGE_ENC_RUN bricks along z of one brick column (bx, by): 8 x 8 rows of up to 32 cells that
// are contiguous in the input.  In pass p lane t reads cell (x = p, y = t >> 5, z = t & 31) - 32 consecutive lanes read 256 consecutive
// bytes - and puts its code into LDS at the cell's place in its brick; then each 512-byte brick leaves as 128 consecutive words from
// consecutive lanes.  Codes follow the lookup table, not first-seen order (nothing observable depends on the numbering): 1 + the first
// matching entry, n_lookup + 1 for a miss that falls to default_material; the grid's first workgroup writes the table that goes with them.
// Box, mask and verdict are reduced per wavefront (shuffles), per workgroup (LDS), then one atomic per word and workgroup.
// One launch serves the batch: a workgroup finds its grid by a search over the descriptors' first_wg.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_grid_encode.h"

using namespace ycge;

namespace {

constexpr int kEncBlock = 256;

__device__ __forceinline__ int morton3(int x, int y, int z)          // VolumeGrid.cs:246-252, as ycge_host.cpp has it
{
    return ((x & 1) << 0) | ((y & 1) << 1) | ((z & 1) << 2) | ((x & 2) << 2) | ((y & 2) << 3) | ((z & 2) << 4) | ((x & 4) << 4) | ((y & 4) << 5) | ((z & 4) << 6);
}

__device__ __forceinline__ int wave_min(int v) { for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(v, s); v = o < v ? o : v; } return v; }
__device__ __forceinline__ int wave_max(int v) { for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(v, s); v = o > v ? o : v; } return v; }
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) { for (int s = 32; s >= 1; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s); v = o < v ? o : v; } return v; }
__device__ __forceinline__ uint32_t wave_or(uint32_t v) { for (int s = 32; s >= 1; s >>= 1) v |= (uint32_t)__shfl_xor((int)v, s); return v; }

__global__ __launch_bounds__(kEncBlock) void k_grid_encode(const GridEncDesc *__restrict__ descs, int n_grids, GridEncResult *__restrict__ results)
{
    __shared__ uint32_t s_codes[YCGE_ENC_RUN * 128];
    __shared__ int32_t s_lookup[2 * YCGE_ENC_MAX_LOOKUP];
    __shared__ int s_lo[3], s_hi[3];
    __shared__ uint32_t s_mask[2], s_bad, s_miss;

    // the grid of this workgroup: the last descriptor whose first_wg <= blockIdx.x (uniform: scalar loads)
    int g = 0;
    for (int lo = 0, hi = n_grids - 1; lo <= hi;) {
        const int mid = (lo + hi) >> 1;
        if (descs[mid].first_wg <= blockIdx.x) { g = mid; lo = mid + 1; } else hi = mid - 1;
    }
    const GridEncDesc D = descs[g];
    const uint32_t local = blockIdx.x - D.first_wg;
    const int bx = (int)(local % (uint32_t)D.nbx), by = (int)((local / (uint32_t)D.nbx) % (uint32_t)D.nby);
    const int bz0 = (int)(local / ((uint32_t)D.nbx * (uint32_t)D.nby)) * YCGE_ENC_RUN;
    const int run = D.nbz - bz0 < YCGE_ENC_RUN ? D.nbz - bz0 : YCGE_ENC_RUN;
    const int t = (int)threadIdx.x;

    for (int k = t; k < D.n_lookup; k += kEncBlock) { s_lookup[2 * k] = D.lookup[3 * k]; s_lookup[2 * k + 1] = D.lookup[3 * k + 1]; }
    if (t < 3) { s_lo[t] = 0x7fffffff; s_hi[t] = -1; }
    if (t == 3) { s_mask[0] = s_mask[1] = 0u; s_bad = 0xffffffffu; s_miss = 0u; }
    if (local == 0) {          // the table that goes with the codes
        int32_t m = -1;
        if (t >= 1 && t <= D.n_lookup) m = D.lookup[3 * (t - 1) + 2];
        else if (t == D.n_lookup + 1 && D.default_material >= 0) m = D.default_material;
        D.lut[t] = m;
    }
    __syncthreads();

    const int ly = t >> 5, lz = t & 31;
    const int iy = by * 8 + ly, iz = bz0 * 8 + lz;
    const bool yz_in = iy < D.ny && iz < D.nz;
    const int brick = ((bz0 + (lz >> 3)) * D.nby + by) * D.nbx + bx;
    int lo_x = 0x7fffffff, hi_x = -1;
    bool solid_any = false;
    uint32_t bad = 0xffffffffu, miss = 0u;
    uint8_t *codes = (uint8_t *)s_codes;
    for (int p = 0; p < 8; p++) {
        const int ix = bx * 8 + p;
        int code = 0;
        if (yz_in && ix < D.nx) {
            const size_t cell = ((size_t)ix * (size_t)D.ny + (size_t)iy) * (size_t)D.nz + (size_t)iz;
            const int2 mm = ((const int2 *)D.cells)[cell];
            if (mm.x > 0) {
                code = -1;
                for (int k = 0; k < D.n_lookup; k++)
                    if (s_lookup[2 * k] == mm.x && s_lookup[2 * k + 1] == mm.y) { code = k + 1; break; }
                if (code < 0) {
                    miss = 1u;
                    if (D.default_material >= 0) code = D.n_lookup + 1;
                    else { code = 0; const uint32_t cc = (uint32_t)cell; bad = cc < bad ? cc : bad; }
                }
                if (code > 0) { solid_any = true; lo_x = ix < lo_x ? ix : lo_x; hi_x = ix > hi_x ? ix : hi_x; }
            }
        }
        codes[(lz >> 3) * 512 + morton3(p, ly, lz & 7)] = (uint8_t)code;
    }

    // per wavefront, then per workgroup
    {
        const int w_lo_x = wave_min(lo_x), w_hi_x = wave_max(hi_x);
        const int w_lo_y = wave_min(solid_any ? iy : 0x7fffffff), w_hi_y = wave_max(solid_any ? iy : -1);
        const int w_lo_z = wave_min(solid_any ? iz : 0x7fffffff), w_hi_z = wave_max(solid_any ? iz : -1);
        const uint32_t bit_lo = (solid_any && D.maskable && brick < 32) ? 1u << brick : 0u;
        const uint32_t bit_hi = (solid_any && D.maskable && brick >= 32 && brick < 64) ? 1u << (brick - 32) : 0u;
        const uint32_t w_mask_lo = wave_or(bit_lo), w_mask_hi = wave_or(bit_hi);
        const uint32_t w_bad = wave_umin(bad), w_miss = wave_or(miss);
        if ((t & 63) == 0) {
            if (w_hi_x >= 0) {
                atomicMin(&s_lo[0], w_lo_x); atomicMax(&s_hi[0], w_hi_x);
                atomicMin(&s_lo[1], w_lo_y); atomicMax(&s_hi[1], w_hi_y);
                atomicMin(&s_lo[2], w_lo_z); atomicMax(&s_hi[2], w_hi_z);
                if (w_mask_lo) atomicOr(&s_mask[0], w_mask_lo);
                if (w_mask_hi) atomicOr(&s_mask[1], w_mask_hi);
            }
            if (w_miss) { atomicOr(&s_miss, 1u); atomicMin(&s_bad, w_bad); }
        }
    }
    __syncthreads();

    // the bricks leave as consecutive words from consecutive lanes
    for (int w = t; w < run * 128; w += kEncBlock) {
        const size_t b = (size_t)(((bz0 + (w >> 7)) * D.nby + by) * D.nbx + bx);
        ((uint32_t *)(D.out + b * 512))[w & 127] = s_codes[w];
    }

    // one atomic per word and workgroup
    GridEncResult *R = results + g;
    if (t < 3 && s_hi[0] >= 0) { atomicMin(&R->lo[t], s_lo[t]); atomicMax(&R->hi[t], s_hi[t]); }
    if (t == 3 && s_mask[0]) atomicOr(&R->mask_lo, s_mask[0]);
    if (t == 4 && s_mask[1]) atomicOr(&R->mask_hi, s_mask[1]);
    if (t == 5 && s_miss) { atomicOr(&R->any_miss, 1u); if (s_bad != 0xffffffffu) atomicMin(&R->bad_cell, s_bad); }
}

}  // namespace

extern "C" int ycge_launch_grid_encode(const void *descs, int n_grids, void *results, uint32_t n_workgroups, hipStream_t stream)
{
    if (n_grids <= 0 || n_workgroups == 0) return 0;
    hipLaunchKernelGGL(k_grid_encode, dim3(n_workgroups), dim3(kEncBlock), 0, stream, (const GridEncDesc *)descs, n_grids, (GridEncResult *)results);
    return (int)hipGetLastError();
}
