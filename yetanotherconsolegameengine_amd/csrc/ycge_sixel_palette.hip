// ycge_sixel_palette.hip - the adaptive sixel palette's kernels (host side: ycge_sixel.cpp; the contract: include/ycge.h at
// ycge_render_frame_sixel_palette; the same rule in plain C++: ycge_sixel_host.cpp).
//
// Everything works from the RGBA8 plane k_sixel_pixels / k_video_pixels wrote, in three launches on the frame's stream:
//   k_pal_hist    the histogram of the 32 768 bins (r >> 3, g >> 3, b >> 3): per bin {pixels, sum r, sum g, sum b}, 16 bytes, zero before
//   k_pal_build   one workgroup: the eight cut passes over the bin-to-box table, then the registers - every box's sums, bytes, sixel
//                 percentages and its definition #i;2;pr;pg;pb at the prefix sum of the definitions' lengths - into the palette block
//   k_pal_remap   the register plane: a pixel's bin through the table
// hold = 1 with a kept palette runs k_pal_remap alone.
//
// The histogram merges before it touches memory.  A lane owns four consecutive pixels (one uint4) and folds equal neighbours; the wavefront
// then takes one slot of its lanes at a time and folds equal bins across lanes: the first pending lane's bin is the leader, the ballot of
// the lanes that hold it is the group, a group of one adds its own entry and a larger one is summed by a butterfly (the other lanes add
// zero) and added by its first lane - four atomics a distinct bin a trip, whatever the picture.  The sums are integers: any order is exact.
//
// The cut passes are level-synchronous inside the one workgroup of 1024 lanes; a lane owns 32 consecutive bins - one (r, g), every b - so
// its bins fold in registers while their box stays the same, and what reaches LDS is one atomic a run: the boxes' occupied bounds (6 words a
// box), then the marginals on the chosen axes (32 words a box), then one lane a box takes the median and the rank of its split, then the
// relabelling.  The table stays in global memory (32 KB, in the cache); LDS holds 39 KB of bounds, marginals and per-box words.
//
// The remap reads the table through the cache, not from LDS: a workgroup would pay 32 KB of loads to fill LDS for 1024 pixels' lookups, and
// a frame at rest touches a few lines of the table.
// The palette block (kPal* offsets below, bytes): the stream's length (the encoder's scan writes it), n, the definitions' length, the 256
// RGBA8 bytes m, the 256 x 3 percentages, the definitions, the table.  Its first kPalReadBack bytes are what a call copies back.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_sixel_host.h"

namespace {

constexpr int kHistBlock = 256;
constexpr int kBuildBlock = 1024;
constexpr uint32_t kBins = ycge_sixel_host::kPaletteBins;
using ycge_sixel_host::kPalCount;
using ycge_sixel_host::kPalDefs;
using ycge_sixel_host::kPalDefsBytes;
using ycge_sixel_host::kPalPct;
using ycge_sixel_host::kPalRgba;
using ycge_sixel_host::kPalTable;

__device__ __forceinline__ uint32_t bin_of(uint32_t word) { return (word & 0xf8u) << 7 | (word >> 11 & 0x1fu) << 5 | (word >> 19 & 0x1fu); }          // word: r | g << 8 | b << 16 | a << 24

// one slot of every lane of the wavefront into the histogram: see above.  Called by all 64 lanes
__device__ __forceinline__ void wave_add(bool pending, uint32_t bin, uint32_t cnt, uint32_t sr, uint32_t sg, uint32_t sb, uint32_t *__restrict__ hist)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(pending);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lead_bin = (uint32_t)__shfl((int)bin, leader, 64);
        const bool mine = pending && bin == lead_bin;
        const unsigned long long group = __ballot(mine);
        if (group & (group - 1ull)) {
            uint32_t c = mine ? cnt : 0u, r = mine ? sr : 0u, g = mine ? sg : 0u, b = mine ? sb : 0u;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                c += (uint32_t)__shfl_xor((int)c, d, 64); r += (uint32_t)__shfl_xor((int)r, d, 64);
                g += (uint32_t)__shfl_xor((int)g, d, 64); b += (uint32_t)__shfl_xor((int)b, d, 64);
            }
            if ((int)lane == leader) { atomicAdd(&hist[4u * lead_bin], c); atomicAdd(&hist[4u * lead_bin + 1u], r); atomicAdd(&hist[4u * lead_bin + 2u], g); atomicAdd(&hist[4u * lead_bin + 3u], b); }
        } else if (mine) {
            atomicAdd(&hist[4u * bin], cnt); atomicAdd(&hist[4u * bin + 1u], sr); atomicAdd(&hist[4u * bin + 2u], sg); atomicAdd(&hist[4u * bin + 3u], sb);
        }
        todo &= ~group;
    }
}

// rgba: n words (16-byte aligned); hist: 4 * 32768 words, zero before the launch.  Every wavefront runs the same number of trips
__global__ __launch_bounds__(kHistBlock) void k_pal_hist(const uint32_t *__restrict__ rgba, uint32_t n, uint32_t *__restrict__ hist)
{
    const uint32_t quads = (n + 3u) / 4u, stride = gridDim.x * kHistBlock;
    const uint32_t trips = (quads + stride - 1u) / stride;
    for (uint32_t t = 0; t < trips; t++) {
        const uint32_t j = t * stride + blockIdx.x * kHistBlock + threadIdx.x;
        uint32_t w[4] = {0, 0, 0, 0};
        uint32_t have = 0;
        if (j < quads) {
            const uint32_t p0 = 4u * j;
            have = n - p0 < 4u ? n - p0 : 4u;
            if (have == 4u) {
                const uint4 q = reinterpret_cast<const uint4 *>(rgba)[j];
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 3; k++)
                    if (k < have) w[k] = rgba[p0 + k];
            }
        }
        uint32_t bin[4], cnt[4], sr[4], sg[4], sb[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            bin[k] = bin_of(w[k]); cnt[k] = k < have ? 1u : 0u;
            sr[k] = w[k] & 0xffu; sg[k] = w[k] >> 8 & 0xffu; sb[k] = w[k] >> 16 & 0xffu;
        }
        // equal neighbours: slot k - 1 moves into slot k
#pragma unroll
        for (uint32_t k = 1; k < 4; k++)
            if (cnt[k] && cnt[k - 1] && bin[k] == bin[k - 1]) {
                cnt[k] += cnt[k - 1]; sr[k] += sr[k - 1]; sg[k] += sg[k - 1]; sb[k] += sb[k - 1];
                cnt[k - 1] = 0;
            }
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) wave_add(cnt[k] != 0u, bin[k], cnt[k], sr[k], sg[k], sb[k], hist);
    }
}

__device__ __forceinline__ uint32_t digits3(uint32_t v) { return 1u + (v >= 10u) + (v >= 100u); }

__device__ __forceinline__ uint32_t put3(uint8_t *s, uint32_t p, uint32_t v)
{
    const uint32_t d = digits3(v);
    for (uint32_t k = d; k-- > 0; v /= 10u) s[p + k] = (uint8_t)('0' + v % 10u);
    return p + d;
}

// One workgroup of 1024 lanes: the palette of the histogram into the block (n, the definitions and their length, the bytes, the percentages,
// the table).  Lane t owns bins 32 t .. 32 t + 31: r = t >> 5, g = t & 31, b = 0..31
__global__ __launch_bounds__(kBuildBlock) void k_pal_build(const uint32_t *__restrict__ hist, uint8_t *__restrict__ block)
{
    __shared__ uint32_t s_lo[256 * 3], s_hi[256 * 3];          // the occupied bounds: min, max + 1 (0: no occupied bin)
    __shared__ uint32_t s_marg[256 * 32];                      // the marginals; behind the passes the boxes' {pixels, sums} and the definitions' offsets
    __shared__ int32_t s_axis[256];                            // the chosen axis, -1: no split
    __shared__ uint32_t s_cut[256], s_label[256];
    __shared__ uint32_t s_n;
    uint8_t *table = block + kPalTable;
    const uint32_t t = threadIdx.x, bin0 = 32u * t;
    const uint32_t coord_r = t >> 5, coord_g = t & 31u;
    uint32_t *table32 = reinterpret_cast<uint32_t *>(table);
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) table32[8u * t + k] = 0u;          // box 0: the whole cube (a lane's own 32 bytes: no other lane reads them)
    uint32_t occupied = 0;                                              // bit b: the lane's bin b holds pixels
    for (uint32_t b = 0; b < 32; b++) occupied |= (uint32_t)(hist[4u * (bin0 + b)] != 0u) << b;
    if (t == 0) s_n = 1;
    __syncthreads();
    for (int pass = 0; pass < 8; pass++) {
        const uint32_t n0 = s_n;
        for (uint32_t k = t; k < 256 * 3; k += kBuildBlock) { s_lo[k] = 32u; s_hi[k] = 0u; }
        for (uint32_t k = t; k < 256 * 32; k += kBuildBlock) s_marg[k] = 0u;
        __syncthreads();
        // the bounds: runs of the lane's occupied bins in one box
        {
            uint32_t box = 0xffffffffu, blo = 32u, bhi = 0u;
            for (uint32_t b = 0; b <= 32; b++) {
                const bool occ = b < 32u && (occupied >> b & 1u);
                const uint32_t bx = occ ? table[bin0 + b] : 0xffffffffu;
                if (b == 32u || (occ && bx != box)) {
                    if (box != 0xffffffffu) {
                        atomicMin(&s_lo[3u * box], coord_r); atomicMax(&s_hi[3u * box], coord_r + 1u);
                        atomicMin(&s_lo[3u * box + 1u], coord_g); atomicMax(&s_hi[3u * box + 1u], coord_g + 1u);
                        atomicMin(&s_lo[3u * box + 2u], blo); atomicMax(&s_hi[3u * box + 2u], bhi);
                    }
                    box = bx; blo = 32u; bhi = 0u;
                }
                if (occ) { blo = blo < b ? blo : b; bhi = b + 1u; }
            }
        }
        __syncthreads();
        if (t < n0) {
            int axis = -1;
            uint32_t best = 0;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const uint32_t lo = s_lo[3u * t + a], hi = s_hi[3u * t + a];
                const uint32_t extent = hi > lo ? hi - 1u - lo : 0u;
                if (extent > best) { best = extent; axis = a; }          // (ties: the first of r, g, b)
            }
            s_axis[t] = axis;
        }
        __syncthreads();
        // the marginals on the chosen axes
        {
            uint32_t box = 0xffffffffu, acc = 0;
            for (uint32_t b = 0; b <= 32; b++) {
                const bool occ = b < 32u && (occupied >> b & 1u);
                const uint32_t bx = occ ? table[bin0 + b] : 0xffffffffu;
                if (b == 32u || (occ && bx != box)) {
                    if (box != 0xffffffffu && acc) atomicAdd(&s_marg[32u * box + (s_axis[box] == 0 ? coord_r : coord_g)], acc);
                    box = bx; acc = 0;
                }
                if (occ) {
                    const int axis = s_axis[bx];
                    const uint32_t c = hist[4u * (bin0 + b)];
                    if (axis == 2) atomicAdd(&s_marg[32u * bx + b], c);
                    else if (axis >= 0) acc += c;
                }
            }
        }
        __syncthreads();
        // one lane a box: the cut, and the new box's index by the rank of the split
        if (t < n0 && s_axis[t] >= 0) {
            const int a = s_axis[t];
            const uint32_t omin = s_lo[3u * t + a], omax = s_hi[3u * t + a] - 1u;
            uint32_t total = 0, acc = 0, cut = omax - 1u;
            for (uint32_t k = omin; k <= omax; k++) total += s_marg[32u * t + k];
            for (uint32_t k = omin; k < omax; k++) {
                acc += s_marg[32u * t + k];
                if (2ull * acc >= total) { cut = k; break; }
            }
            uint32_t rank = 0;
            for (uint32_t b = 0; b < t; b++) rank += s_axis[b] >= 0;
            s_cut[t] = cut; s_label[t] = n0 + rank;
        }
        __syncthreads();
        // the relabelling: every bin of a split box beyond its cut, empty bins included
        for (uint32_t b = 0; b < 32; b++) {
            const uint32_t bx = table[bin0 + b];
            const int axis = s_axis[bx];
            if (axis < 0) continue;
            const uint32_t c = axis == 0 ? coord_r : axis == 1 ? coord_g : b;
            if (c > s_cut[bx]) table[bin0 + b] = (uint8_t)s_label[bx];
        }
        if (t == 0) {
            uint32_t splits = 0;
            for (uint32_t b = 0; b < n0; b++) splits += s_axis[b] >= 0;
            s_n = n0 + splits;
        }
        __syncthreads();
    }
    // the registers: every box's pixels and sums (runs of the lane's bins in one box, one atomic a run and channel)
    const uint32_t n = s_n;
    for (uint32_t k = t; k < 256 * 4; k += kBuildBlock) s_marg[k] = 0u;
    __syncthreads();
    {
        uint32_t box = 0xffffffffu, c = 0, r = 0, g = 0, bl = 0;
        for (uint32_t b = 0; b <= 32; b++) {
            const bool occ = b < 32u && (occupied >> b & 1u);
            const uint32_t bx = occ ? table[bin0 + b] : 0xffffffffu;
            if (b == 32u || (occ && bx != box)) {
                if (box != 0xffffffffu) { atomicAdd(&s_marg[4u * box], c); atomicAdd(&s_marg[4u * box + 1u], r); atomicAdd(&s_marg[4u * box + 2u], g); atomicAdd(&s_marg[4u * box + 3u], bl); }
                box = bx; c = r = g = bl = 0;
            }
            if (occ) {
                const uint4 h = reinterpret_cast<const uint4 *>(hist)[bin0 + b];
                c += h.x; r += h.y; g += h.z; bl += h.w;
            }
        }
    }
    __syncthreads();
    // lanes 0..255: register t's bytes, percentages and definition; the definitions' offsets by a serial prefix over at most 256 lengths
    uint32_t pct[3] = {0, 0, 0}, len = 0;
    if (t < 256u) {
        uint32_t word = 0;
        if (t < n) {
            const unsigned long long k = s_marg[4u * t];
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const unsigned long long m = k ? (2ull * s_marg[4u * t + 1u + ch] + k) / (2ull * k) : 0ull;
                word |= (uint32_t)m << (8 * ch);
                pct[ch] = (uint32_t)((200ull * m + 255ull) / 510ull);
            }
            word |= 0xff000000u;
            len = 1u + digits3(t) + 3u + digits3(pct[0]) + 1u + digits3(pct[1]) + 1u + digits3(pct[2]);
        }
        reinterpret_cast<uint32_t *>(block + kPalRgba)[t] = word;
        block[kPalPct + 3u * t] = (uint8_t)pct[0]; block[kPalPct + 3u * t + 1u] = (uint8_t)pct[1]; block[kPalPct + 3u * t + 2u] = (uint8_t)pct[2];
        s_cut[t] = len;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < 256u; k++) { const uint32_t l = s_cut[k]; s_label[k] = at; at += l; }
        *reinterpret_cast<uint32_t *>(block + kPalCount) = n;
        *reinterpret_cast<uint32_t *>(block + kPalDefsBytes) = at;
    }
    __syncthreads();
    if (t < n) {
        uint8_t *s = block + kPalDefs;
        uint32_t p = s_label[t];
        s[p++] = (uint8_t)'#';
        p = put3(s, p, t);
        s[p++] = (uint8_t)';'; s[p++] = (uint8_t)'2'; s[p++] = (uint8_t)';';
        p = put3(s, p, pct[0]); s[p++] = (uint8_t)';';
        p = put3(s, p, pct[1]); s[p++] = (uint8_t)';';
        p = put3(s, p, pct[2]);
    }
}

// the register plane of n pixels through the table: a lane four pixels, one word stored; the last lane of an n that is no multiple of 4
// stores byte by byte
__global__ __launch_bounds__(kHistBlock) void k_pal_remap(const uint32_t *__restrict__ rgba, uint32_t n, const uint8_t *__restrict__ table, uint8_t *__restrict__ index)
{
    const uint32_t quads = (n + 3u) / 4u, stride = gridDim.x * kHistBlock;
    for (uint32_t j = blockIdx.x * kHistBlock + threadIdx.x; j < quads; j += stride) {
        const uint32_t p0 = 4u * j;
        if (n - p0 >= 4u) {
            const uint4 q = reinterpret_cast<const uint4 *>(rgba)[j];
            const uint32_t a = table[bin_of(q.x)], b = table[bin_of(q.y)], c = table[bin_of(q.z)], d = table[bin_of(q.w)];
            reinterpret_cast<uint32_t *>(index)[j] = a | b << 8 | c << 16 | d << 24;
        } else {
            for (uint32_t k = p0; k < n; k++) index[k] = table[bin_of(rgba[k])];
        }
    }
}

} // namespace

extern "C" {

// The palette stage on an RGBA plane of n = W * H <= 2^24 pixels (16-byte aligned).  build != 0: hist (4 * 32768 words) is cleared and
// filled, k_pal_build writes the block; then the register plane through the block's table (index: n bytes, 4-byte aligned; NULL: none)
int ycge_launch_sixel_palette(const uint8_t *rgba, int W, int H, int build, uint32_t *hist, uint8_t *block, uint8_t *index, int compute_units, hipStream_t stream)
{
    if (!rgba || !block || (build && !hist) || W <= 0 || H <= 0 || (int64_t)W * H > ((int64_t)1 << 24) || ((uintptr_t)rgba & 15u) || ((uintptr_t)block & 15u) ||
        ((uintptr_t)index & 3u) || ((uintptr_t)hist & 15u))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)W * (uint32_t)H;
    const uint32_t need = ((n + 3u) / 4u + kHistBlock - 1) / kHistBlock;
    const uint32_t limit = (uint32_t)(compute_units > 0 ? compute_units : 256) * 8u;
    const dim3 grid(need < limit ? need : limit);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(rgba);
    if (build) {
        const hipError_t e = hipMemsetAsync(hist, 0, (size_t)4 * kBins * sizeof(uint32_t), stream);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_pal_hist, grid, dim3(kHistBlock), 0, stream, words, n, hist);
        hipLaunchKernelGGL(k_pal_build, dim3(1), dim3(kBuildBlock), 0, stream, hist, block);
    }
    if (index) hipLaunchKernelGGL(k_pal_remap, grid, dim3(kHistBlock), 0, stream, words, n, block + kPalTable, index);
    return (int)hipGetLastError();
}

} // extern "C"
