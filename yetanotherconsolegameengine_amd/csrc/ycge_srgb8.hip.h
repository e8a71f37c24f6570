// ycge_srgb8.hip.h - LinearToSrgb8 on the device, the one body of k_encode_chexels, k_fit_quadrants (ycge_chexel.hip) and k_sixel_pixels
// (ycge_sixel.hip).  The byte is the number of the host's thresholds (ycge_chexel.cpp, SrgbTables) that are <= x: no device pow decides one.
#pragma once
#include <hip/hip_runtime.h>

namespace ycge_chexel {

// Clamp01 (Chexel.cs:92-98): compare in double, NaN and -0.0 pass unchanged; the result is a binary32 again (Vec3's fields)
__device__ __forceinline__ float clamp01(float x) { return (double)x < 0.0 ? 0.0f : ((double)x > 1.0 ? 1.0f : x); }

// the number of thresholds <= x: a branchless search over the 255 sorted entries (entry 255 is never read)
template <class T>
__device__ __forceinline__ int srgb8(const T *t, T x)
{
    int pos = 0;
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) pos += t[pos + s - 1] <= x ? s : 0;
    return pos;
}

} // namespace ycge_chexel
