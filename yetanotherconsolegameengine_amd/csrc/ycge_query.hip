// ycge_query.hip - the kernel of the scene queries (ycge_scene_hit / ycge_scene_occluded; host side: ycge_query.cpp).
//
// Its own translation unit: the walk is the frames' own (ycge_rt.hip.h: traverse, resolve_hit - included, not copied), and the code
// objects of ycge_kernels.hip stay exactly what they were (the same kernels compiled next to k_query got one more VGPR in k_trace and
// k_trace_batch - the counting k_trace_batch lost a wavefront per SIMD).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ycge_rt.hip.h"

namespace ycge {

// ---------------------------------------------------------------------------------- scene queries (ycge_scene_hit / ycge_scene_occluded)
// Scene.Hit (Scene.cs:71-75) for a batch of caller rays: one lane per ray, a bounded grid of resident wavefronts walks the batch by grid
// stride (the spill area is sized for those lanes, not for the batch).  The walk is the frames' own: traverse() from the scene root
// (the generic walk handles every root kind) and resolve_hit() for the record.  OCCLUDED: the boolean of Scene.Hit only - the walk
// stops at the first accepted hit, which is exact for the boolean (the traversal is identical up to it).
// A ray the reference could not trace (a non-finite origin / direction / tMin, a NaN tMax, a direction whose squared length is not a
// finite positive binary32) is refused: its index goes to *first_bad by atomic min and the host reports the first one.
struct QueryArgs {
    const float4 *rays;       // n x {ox oy oz dx, dy dz tmin tmax}
    float *hits;              // n x 10 {t, p xyz, n xyz, albedo rgb}   (closest hit)
    int32_t *ids;             // n x 2 {object, sub}                     (closest hit)
    uint8_t *occluded;        // n                                       (OCCLUDED)
    uint32_t *first_bad;      // UINT32_MAX on entry
    void *spill;
    uint32_t n, lanes;        // lanes = the grid's threads (the spill area's columns)
};
template <bool HAS_GRID, bool OCCLUDED>
__global__ __launch_bounds__(64) void k_query(const SceneDev S, const QueryArgs A)
{
    Work w = {0, 0, 0, 0, 0, 0, 0};
    StackT<64> st;
    st.init(A.spill, A.lanes);
    for (uint32_t i = blockIdx.x * 64u + threadIdx.x; i < A.n; i += A.lanes) {
        const float4 a = A.rays[2 * (size_t)i], b = A.rays[2 * (size_t)i + 1];
        const float len_sq = a.w * a.w + b.x * b.x + b.y * b.y;
        const bool ok = isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(a.w) && isfinite(b.x) && isfinite(b.y) && isfinite(b.z) &&
                        !isnan(b.w) && isfinite(len_sq) && len_sq > 0.0f;
        float t = 0.0f;
        int prim = -1, sub = 0;
        RayQ q;
        if (ok) {
            q.o = f3(a.x, a.y, a.z);
            q.d = normalized(f3(a.w, b.x, b.y));      // new Ray(o, d), Ray.cs:8-12
            q.tmin = b.z; q.tmax = b.w;
            q.anyhit = OCCLUDED;
            traverse<false, HAS_GRID, false>(S, q, st, t, prim, sub, w);
        } else {
            atomicMin(A.first_bad, i);
        }
        if (OCCLUDED) {
            A.occluded[i] = prim >= 0 ? 1 : 0;
        } else {
            float *r = A.hits + (size_t)i * 10;
            if (prim >= 0) {
                HitAttr h;
                resolve_hit<HAS_GRID>(S, prim, sub, t, q.o, q.d, h);
                r[0] = t; r[1] = h.p.x; r[2] = h.p.y; r[3] = h.p.z; r[4] = h.n.x; r[5] = h.n.y; r[6] = h.n.z;
                r[7] = h.m.albedo.x; r[8] = h.m.albedo.y; r[9] = h.m.albedo.z;
                A.ids[2 * (size_t)i] = prim; A.ids[2 * (size_t)i + 1] = h.sub_public;
            } else {
                for (int k = 0; k < 10; k++) r[k] = 0.0f;
                A.ids[2 * (size_t)i] = -1; A.ids[2 * (size_t)i + 1] = -1;
            }
        }
    }
}

} // namespace ycge

namespace {
template <class F> void sel2(bool a, bool b, F f)
{
    using T = std::true_type; using N = std::false_type;
    if (a) { if (b) f(T{}, T{}); else f(T{}, N{}); }
    else { if (b) f(N{}, T{}); else f(N{}, N{}); }
}
} // namespace

extern "C" {

// scene queries (k_query): the threads of a grid that is resident at once on `compute_units` CUs - the lanes that walk a batch and the
// columns of its spill area
uint32_t ycge_launch_query_lanes(int has_grid, int occluded, int compute_units)
{
    using namespace ycge;
    int per_cu = 0;
    hipError_t e = hipErrorInvalidValue;
    sel2(has_grid != 0, occluded != 0, [&](auto G, auto O) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_query<decltype(G)::value, decltype(O)::value>, 64, 0);
    });
    if (e != hipSuccess || per_cu <= 0) { (void)hipGetLastError(); per_cu = 8; }
    if (per_cu > 16) per_cu = 16;           // four wavefronts per SIMD: the spill area stays 16 MB per level of depth beyond the LDS part on 256 CUs
    return (uint32_t)(compute_units > 0 ? compute_units : 1) * (uint32_t)per_cu * 64u;
}
// n rays (n >= 1) on `lanes` threads (a multiple of 64, at most what ycge_launch_query_lanes gave: the spill area's columns)
int ycge_launch_query(const ycge::SceneDev *S, const float *rays, uint32_t n, float *hits, int32_t *ids, uint8_t *occluded, uint32_t *first_bad,
                      void *spill, uint32_t lanes, int has_grid, hipStream_t stream)
{
    using namespace ycge;
    if (n == 0) return 0;
    const uint32_t need = (n + 63u) / 64u * 64u;
    QueryArgs A;
    A.rays = (const float4 *)rays; A.hits = hits; A.ids = ids; A.occluded = occluded; A.first_bad = first_bad; A.spill = spill;
    A.n = n; A.lanes = need < lanes ? need : lanes;
    const dim3 grid(A.lanes / 64u), block(64);
    sel2(has_grid != 0, occluded != nullptr, [&](auto G, auto O) {
        hipLaunchKernelGGL((k_query<decltype(G)::value, decltype(O)::value>), grid, block, 0, stream, *S, A);
    });
    return (int)hipGetLastError();
}

} // extern "C"
