// ycge_grid_edit.hip - voxel edits of resident grids on the device (host side: ycge_grid_edit.cpp).  Its own translation unit, as
// ycge_grid_encode.hip is: the code objects of the frame kernels and of k_grid_encode stay what they were.
//
//   k_grid_edit   one workgroup of 128 lanes per touched brick (GridEditRecord).  A brick is 512 bytes in Morton order, so lane t owns
//                 word t: the four cells (x0 | 0..1, y0 | 0..1, z0) - bits 0 and 1 of a Morton index are x's and y's lowest - whose other
//                 bits the lane unpacks from t once.  It reads its word, walks the grid's ops in list order (records and ops are read
//                 at workgroup-uniform addresses: scalar loads; an op whose box misses the brick is skipped by a uniform branch),
//                 replaces the bytes the box covers, and stores the word only if it differs.  No two lanes write one word: no atomics
//                 on cells, no LDS but two counters, no scratch.  Changed cells are summed per wavefront (shuffles), per workgroup
//                 (LDS), then one atomic per counter and workgroup: counters[0] += cells whose byte differs from before the call,
//                 counters[1] += 1 for a brick that holds one.
//   k_grid_solid  for every edited grid the index box of its non-zero codes and its brick mask, into a GridEncResult, in k_grid_encode's
//                 order: per wavefront, per workgroup, one atomic per word and workgroup.  A workgroup of 256 lanes takes two bricks,
//                 a lane one word; a wavefront lies inside one brick.  Padding cells of partial bricks are zero and contribute nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_grid_edit.h"

using namespace ycge;

namespace {

constexpr int kEditBlock = 128, kSolidBlock = 256;

__device__ __forceinline__ int wave_min(int v) { for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(v, s); v = o < v ? o : v; } return v; }
__device__ __forceinline__ int wave_max(int v) { for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(v, s); v = o > v ? o : v; } return v; }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s); return v; }
__device__ __forceinline__ uint32_t wave_or(uint32_t v) { for (int s = 32; s >= 1; s >>= 1) v |= (uint32_t)__shfl_xor((int)v, s); return v; }

// word w of a brick: the cell of its byte 0 (morton3 of ycge_grid_encode.hip undone for m = 4 w; bytes 1..3 are x + 1, y + 1, both)
__device__ __forceinline__ void word_cell(int w, int &x, int &y, int &z)
{
    x = ((w >> 1) & 1) << 1 | ((w >> 4) & 1) << 2;
    y = ((w >> 2) & 1) << 1 | ((w >> 5) & 1) << 2;
    z = (w & 1) | ((w >> 3) & 1) << 1 | ((w >> 6) & 1) << 2;
}

__global__ __launch_bounds__(kEditBlock) void k_grid_edit(uint8_t *__restrict__ arena, const GridEditRecord *__restrict__ records, const GridEditOp *__restrict__ ops,
                                                          uint32_t *__restrict__ counters)
{
    __shared__ uint32_t s_changed;
    const GridEditRecord R = records[blockIdx.x];
    const int t = (int)threadIdx.x;
    if (t == 0) s_changed = 0u;
    __syncthreads();
    int x, y, z;
    word_cell(t, x, y, z);
    x += R.bx * 8; y += R.by * 8; z += R.bz * 8;
    uint32_t *word = (uint32_t *)(arena + R.brick) + t;
    const uint32_t before = *word;
    uint32_t now = before;
    const int bx0 = R.bx * 8, by0 = R.by * 8, bz0 = R.bz * 8;
    for (uint32_t k = 0; k < R.op_count; k++) {
        const GridEditOp op = ops[R.op_first + k];
        if (op.hi[0] < bx0 || op.lo[0] > bx0 + 7 || op.hi[1] < by0 || op.lo[1] > by0 + 7 || op.hi[2] < bz0 || op.lo[2] > bz0 + 7) continue;          // (uniform)
        if (z < op.lo[2] || z > op.hi[2]) continue;
        const bool x0 = x >= op.lo[0] && x <= op.hi[0], x1 = x + 1 >= op.lo[0] && x + 1 <= op.hi[0];
        const bool y0 = y >= op.lo[1] && y <= op.hi[1], y1 = y + 1 >= op.lo[1] && y + 1 <= op.hi[1];
        const uint32_t mask = (x0 && y0 ? 0x000000ffu : 0u) | (x1 && y0 ? 0x0000ff00u : 0u) | (x0 && y1 ? 0x00ff0000u : 0u) | (x1 && y1 ? 0xff000000u : 0u);
        now = (now & ~mask) | ((op.code * 0x01010101u) & mask);
    }
    const uint32_t diff = now ^ before;
    if (diff) *word = now;
    const uint32_t changed = ((diff & 0xffu) != 0u) + ((diff & 0xff00u) != 0u) + ((diff & 0xff0000u) != 0u) + ((diff & 0xff000000u) != 0u);
    const uint32_t w_changed = wave_sum(changed);
    if ((t & 63) == 0 && w_changed) atomicAdd(&s_changed, w_changed);
    __syncthreads();
    if (t == 0 && s_changed) { atomicAdd(&counters[0], s_changed); atomicAdd(&counters[1], 1u); }
}

__global__ __launch_bounds__(kSolidBlock) void k_grid_solid(const uint8_t *__restrict__ arena, const GridSolidDesc *__restrict__ descs, int n_grids, GridEncResult *__restrict__ results)
{
    __shared__ int s_lo[3], s_hi[3];
    __shared__ uint32_t s_mask[2];
    // the grid of this workgroup: the last descriptor whose first_wg <= blockIdx.x (uniform: scalar loads)
    int g = 0;
    for (int lo = 0, hi = n_grids - 1; lo <= hi;) {
        const int mid = (lo + hi) >> 1;
        if (descs[mid].first_wg <= blockIdx.x) { g = mid; lo = mid + 1; } else hi = mid - 1;
    }
    const GridSolidDesc D = descs[g];
    const int t = (int)threadIdx.x;
    if (t < 3) { s_lo[t] = 0x7fffffff; s_hi[t] = -1; }
    if (t == 3) s_mask[0] = s_mask[1] = 0u;
    __syncthreads();

    const int brick = (int)(blockIdx.x - D.first_wg) * 2 + (t >> 7);          // (wavefront-uniform)
    int lo_x = 0x7fffffff, hi_x = -1, lo_y = 0x7fffffff, hi_y = -1, z_any = -1;
    if (brick < D.n_bricks) {
        const uint32_t word = ((const uint32_t *)(arena + D.cells + (size_t)brick * 512))[t & 127];
        if (word) {
            const int bx = brick % D.nbx, by = (brick / D.nbx) % D.nby, bz = brick / (D.nbx * D.nby);
            int x, y, z;
            word_cell(t & 127, x, y, z);
            x += bx * 8; y += by * 8; z_any = z + bz * 8;
            const bool c0 = (word & 0xffu) != 0u, c1 = (word & 0xff00u) != 0u, c2 = (word & 0xff0000u) != 0u, c3 = (word & 0xff000000u) != 0u;
            lo_x = (c0 || c2) ? x : x + 1; hi_x = (c1 || c3) ? x + 1 : x;
            lo_y = (c0 || c1) ? y : y + 1; hi_y = (c2 || c3) ? y + 1 : y;
        }
    }
    // per wavefront, then per workgroup
    {
        const bool any = z_any >= 0;
        const int w_lo_x = wave_min(lo_x), w_hi_x = wave_max(hi_x), w_lo_y = wave_min(lo_y), w_hi_y = wave_max(hi_y);
        const int w_lo_z = wave_min(any ? z_any : 0x7fffffff), w_hi_z = wave_max(z_any);
        const uint32_t w_mask_lo = wave_or((any && D.maskable && brick < 32) ? 1u << brick : 0u);
        const uint32_t w_mask_hi = wave_or((any && D.maskable && brick >= 32 && brick < 64) ? 1u << (brick - 32) : 0u);
        if ((t & 63) == 0 && w_hi_x >= 0) {
            atomicMin(&s_lo[0], w_lo_x); atomicMax(&s_hi[0], w_hi_x);
            atomicMin(&s_lo[1], w_lo_y); atomicMax(&s_hi[1], w_hi_y);
            atomicMin(&s_lo[2], w_lo_z); atomicMax(&s_hi[2], w_hi_z);
            if (w_mask_lo) atomicOr(&s_mask[0], w_mask_lo);
            if (w_mask_hi) atomicOr(&s_mask[1], w_mask_hi);
        }
    }
    __syncthreads();
    // one atomic per word and workgroup
    GridEncResult *R = results + g;
    if (t < 3 && s_hi[0] >= 0) { atomicMin(&R->lo[t], s_lo[t]); atomicMax(&R->hi[t], s_hi[t]); }
    if (t == 3 && s_mask[0]) atomicOr(&R->mask_lo, s_mask[0]);
    if (t == 4 && s_mask[1]) atomicOr(&R->mask_hi, s_mask[1]);
}

}  // namespace

extern "C" int ycge_launch_grid_edit(uint8_t *arena, const void *records, uint32_t n_records, const void *ops, uint32_t *counters, hipStream_t stream)
{
    if (n_records == 0) return 0;
    if (n_records > YCGE_EDIT_MAX_RECORDS) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_grid_edit, dim3(n_records), dim3(kEditBlock), 0, stream, arena, (const GridEditRecord *)records, (const GridEditOp *)ops, counters);
    return (int)hipGetLastError();
}

extern "C" int ycge_launch_grid_solid(const uint8_t *arena, const void *descs, int n_grids, void *results, uint32_t n_workgroups, hipStream_t stream)
{
    if (n_grids <= 0 || n_workgroups == 0) return 0;
    hipLaunchKernelGGL(k_grid_solid, dim3(n_workgroups), dim3(kSolidBlock), 0, stream, arena, (const GridSolidDesc *)descs, n_grids, (GridEncResult *)results);
    return (int)hipGetLastError();
}
