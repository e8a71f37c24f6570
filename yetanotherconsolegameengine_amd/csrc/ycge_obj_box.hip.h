// ycge_obj_box.hip.h - min / max of floats over a launch, exact whatever the order of arrival: the two-stage ordered-integer reduction of
// k_obj_bounds and k_obj_triangles (ycge_obj.hip) and of k_ground_bounds (ycge_obj_ground.hip).  -0 orders below +0, NaN never replaces an
// extreme.  A box is six words, min xyz then max xyz, cleared to 0xffffffff x 3, 0 x 3; lo > hi: nothing grew it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// a float as an unsigned integer of the same order (-0 below +0); and back
__device__ __forceinline__ uint32_t ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// this lane's box (ordered integers; lo > hi: nothing) into the workgroup's in LDS, then into box[6] by one atomic per component
__device__ __forceinline__ void reduce_box(const uint32_t lo[3], const uint32_t hi[3], uint32_t *__restrict__ box)
{
    __shared__ uint32_t sbox[6];
    if (threadIdx.x < 3) { sbox[threadIdx.x] = 0xffffffffu; sbox[3 + threadIdx.x] = 0u; }
    __syncthreads();
    for (int a = 0; a < 3; a++) {
        if (lo[a] <= hi[a]) { atomicMin(&sbox[a], lo[a]); atomicMax(&sbox[3 + a], hi[a]); }
    }
    __syncthreads();
    if (threadIdx.x < 3) { if (sbox[threadIdx.x] <= sbox[3 + threadIdx.x]) { atomicMin(&box[threadIdx.x], sbox[threadIdx.x]); atomicMax(&box[3 + threadIdx.x], sbox[3 + threadIdx.x]); } }
}

__device__ __forceinline__ void grow(uint32_t lo[3], uint32_t hi[3], const float p[3])
{
    for (int a = 0; a < 3; a++) {
        if (p[a] != p[a]) continue;
        const uint32_t o = ordered(p[a]);
        lo[a] = o < lo[a] ? o : lo[a];
        hi[a] = o > hi[a] ? o : hi[a];
    }
}

} // namespace
