// ycge_bvh_build.hip - the scene-level BVH (Objects/BVH.cs:258-459) built ON THE DEVICE, for ycge_scene_update_objects
// (Scene.RebuildBVH when an entity moved, Scenes/Scene.cs:122-127): same topology, node numbering and leaf order as the
// reference's recursive builder - the host builder in ycge_accel.cpp is the sequential statement of the same thing and
// what the parity tests compare this against, node for node.
//
// One 1024-thread workgroup on one CU.  A node is split by ONE wavefront (items in chunks of 64); nodes wait in an LDS
// queue that the 16 wavefronts pop from, so subtrees are built side by side.  Everything order-dependent in the reference
// is reproduced exactly:
//   * binning (BVH.cs:322-352): counts are integer sums, bin boxes and centroid bounds are min / max - order-free (LDS
//     atomics on order-preserving integer keys).  The one thing an order could change is the sign of a zero bound, which
//     reaches only the SAH cost's sign of zero and no comparison;
//   * the SAH sweep (16 bins, strict '<' over axes then bins): running boxes and counts by scans over the bins (min / max / integer
//     sums), the cost of every split by one lane with the reference's operation order, first minimum in (axis, bin) order wins;
//   * the partition (BVH.cs:394-410) is the reference's two-pointer in-place loop, whose RESULT depends on the order the
//     items are visited in.  It has a closed form (tests/test_partition_closed_form.py checks it exhaustively): with
//     mid = #L, the front region = positions < mid plus position mid if it holds an R, the back region = the rest;
//       - a front L stays; the k-th front R (ascending) goes to slot e if k = 1, else to (position of the (k-1)-th back L,
//         counted from the end) - 1, and its slot - if below mid - receives the k-th back L;
//       - a back R moves down by one slot;
//     so one prefix count and one small index list give every item its slot in parallel;
//   * nodes are numbered in pre-order afterwards from subtree sizes (a node's children were created after it).
//   * the degenerate cases the reference hands to Array.Sort (no valid split, or a partition that leaves one side empty -
//     config 5's chunk lattice has them in every build) run the same introsort restatement as the host builder
//     (ycge_keysort.h), every lane of the wavefront in step on the one LDS slice, keys cached in LDS.
// `fallback` is left for a tree deeper than the reference's 128-entry stack: the host builder redoes it and reports the error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "ycge_bvh_split.hip.h"

namespace ycge {

// items: nine planes of n floats - box min x, y, z, box max x, y, z, centroid x, y, z (what Scene.RebuildBVH gets from
// Hittable.TryGetBounds, BVH.cs:32-53).  Outputs: ref_out = the reference-format nodes in pre-order (ycge_read_accel),
// gnodes_out = the traversal records of the inner nodes in their own pre-order, leaf_out = leafObjIndex, res.
__global__ __launch_bounds__(1024) void k_scene_bvh_build(const float *__restrict__ items, const int n, BvhBuildNode *__restrict__ nodes,
                                                          RefNodeDev *__restrict__ ref_out, GNode *__restrict__ gnodes_out,
                                                          uint32_t *__restrict__ leaf_out, BvhBuildResult *__restrict__ res, const int active_waves)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bvh_lds[];      // above the 64 KB a static allocation may take
    BvhShared &sh = *reinterpret_cast<BvhShared *>(bvh_lds);
    const int tid = (int)threadIdx.x, lane = tid & 63;
    for (int i = tid; i < n; i += 1024) sh.ord[i] = (uint16_t)i;
    for (int i = tid; i < YCGE_BVH_DEV_MAX_ITEMS; i += 1024) sh.queue[i] = 0ull;
    if (tid == 0) {
        sh.q_head = 0; sh.q_tail = 0; sh.pending = 0; sh.n_nodes = 1; sh.fallback = 0; sh.max_depth = 1; sh.sorts = 0;
        BvhBuildNode &r = nodes[0];
        r.start = 0; r.count = n; r.depth = 1; r.left = -1; r.inner = 0; r.pre = 0; r.ipre = 0;
        if (n > YCGE_BVH_DEV_LEAF) {
            sh.pending = 1; sh.q_tail = 1;
            sh.queue[0] = (1ull << 63) | (1ull << 48) | ((unsigned long long)n << 32);
        }
    }
    __syncthreads();
    bvh_build_loop<false>(sh, items, n, nodes, active_waves);
    __syncthreads();
    const int n_nodes = (int)sh.n_nodes, max_depth = (int)sh.max_depth;
    if (sh.fallback) {
        if (tid == 0) { res->fallback = 1; res->n_nodes = 0; res->n_inner = 0; res->max_depth = 0; res->root_ref = YCGE_REF_NONE_VALUE; }
        return;
    }
    // ---- leaf boxes (compare-assign in leaf order, BVH.cs:281-296), then inner boxes and subtree sizes bottom-up
    for (int i = tid; i < n_nodes; i += 1024) {
        BvhBuildNode &nd = nodes[i];
        if (nd.left >= 0) continue;
        float mn[3], mx[3];
        const int first = sh.ord[nd.start];
        for (int k = 0; k < 3; k++) { mn[k] = items[(size_t)k * n + first]; mx[k] = items[(size_t)(3 + k) * n + first]; }
        for (int j = 1; j < nd.count; j++) {
            const int it = sh.ord[nd.start + j];
            for (int k = 0; k < 3; k++) { const float v = items[(size_t)k * n + it]; if (v < mn[k]) mn[k] = v; }
            for (int k = 0; k < 3; k++) { const float v = items[(size_t)(3 + k) * n + it]; if (v > mx[k]) mx[k] = v; }
        }
        for (int k = 0; k < 3; k++) { nd.mn[k] = mn[k]; nd.mx[k] = mx[k]; }
        nd.inner = 0;
    }
    __syncthreads();
    for (int d = max_depth - 1; d >= 1; d--) {
        for (int i = tid; i < n_nodes; i += 1024) {
            BvhBuildNode &nd = nodes[i];
            if (nd.left < 0 || nd.depth != d) continue;
            const BvhBuildNode &L = nodes[nd.left], &R = nodes[nd.left + 1];
            for (int k = 0; k < 3; k++) { nd.mn[k] = cs_min(L.mn[k], R.mn[k]); nd.mx[k] = cs_max(L.mx[k], R.mx[k]); }      // MathF.Min / Max, BVH.cs:438-443
            nd.inner = 1 + L.inner + R.inner;
        }
        __syncthreads();
    }
    // ---- pre-order numbers top-down: left child next, right child after the left subtree (2 inner + 1 nodes)
    for (int d = 1; d < max_depth; d++) {
        for (int i = tid; i < n_nodes; i += 1024) {
            BvhBuildNode &nd = nodes[i];
            if (nd.left < 0 || nd.depth != d) continue;
            BvhBuildNode &L = nodes[nd.left], &R = nodes[nd.left + 1];
            L.pre = nd.pre + 1; L.ipre = nd.ipre + 1;
            R.pre = nd.pre + 1 + 2 * L.inner + 1; R.ipre = nd.ipre + 1 + L.inner;
        }
        __syncthreads();
    }
    for (int i = tid; i < n_nodes; i += 1024) {
        const BvhBuildNode &nd = nodes[i];
        RefNodeDev o;
        for (int k = 0; k < 3; k++) { o.mn[k] = nd.mn[k]; o.mx[k] = nd.mx[k]; }
        if (nd.left < 0) { o.left = o.right = -1; o.start = nd.start; o.count = nd.count; }
        else {
            const BvhBuildNode &L = nodes[nd.left], &R = nodes[nd.left + 1];
            o.left = L.pre; o.right = R.pre; o.start = 0; o.count = 0;
            GNode g;
            g.lmin_x = L.mn[0]; g.lmin_y = L.mn[1]; g.lmin_z = L.mn[2]; g.lmax_x = L.mx[0]; g.lmax_y = L.mx[1]; g.lmax_z = L.mx[2];
            g.rmin_x = R.mn[0]; g.rmin_y = R.mn[1]; g.rmin_z = R.mn[2]; g.rmax_x = R.mx[0]; g.rmax_y = R.mx[1]; g.rmax_z = R.mx[2];
            g.lref = L.left < 0 ? YCGE_REF(REF_SCENE_LEAF, ((uint32_t)L.start << 3) | (uint32_t)L.count) : YCGE_REF(REF_SCENE_NODE, (uint32_t)L.ipre);
            g.rref = R.left < 0 ? YCGE_REF(REF_SCENE_LEAF, ((uint32_t)R.start << 3) | (uint32_t)R.count) : YCGE_REF(REF_SCENE_NODE, (uint32_t)R.ipre);
            g.pad[0] = g.pad[1] = 0;
            gnodes_out[nd.ipre] = g;
        }
        ref_out[nd.pre] = o;
    }
    for (int i = tid; i < n; i += 1024) leaf_out[i] = sh.ord[i];
    if (tid == 0) {
        const BvhBuildNode &r = nodes[0];
        res->fallback = 0; res->n_nodes = n_nodes; res->n_inner = r.inner; res->max_depth = max_depth; res->sorts = sh.sorts;
        res->root_ref = r.left < 0 ? YCGE_REF(REF_SCENE_LEAF, ((uint32_t)r.start << 3) | (uint32_t)r.count) : YCGE_REF(REF_SCENE_NODE, 0u);
        for (int k = 0; k < 3; k++) { res->root_min[k] = r.mn[k]; res->root_max[k] = r.mx[k]; }
    }
}


// ---------------------------------------------------------------------------------- SceneDev::walk_nodes
// The walk tree of a world of voxel grids (ycge_device.h, SceneDev::walk_nodes) from whichever scene tree is installed: entry i < n is
// scene node i with its child references rewritten, and each leaf child of 2..7 objects gets the YCGE_WALK_LEAF_NODES entries from
// n + (2 i + side) * YCGE_WALK_LEAF_NODES on for its own nodes (a leaf of k objects uses k - 1).  One thread per (node, side): a leaf's
// nodes depend on its own objects only.
struct SolidBox { float lo[3], hi[3]; };
__device__ __forceinline__ SolidBox solid_of(const GPrim &g)
{
    const float inf = __builtin_huge_valf();
    SolidBox b;
    if (g.type == 10) { for (int a = 0; a < 3; a++) { b.lo[a] = g.p[a]; b.hi[a] = g.p[3 + a]; } }
    else { for (int a = 0; a < 3; a++) { b.lo[a] = -inf; b.hi[a] = inf; } }
    return b;
}
__device__ __forceinline__ uint32_t walk_ref_of(const GPrim &g, uint32_t prim) { return g.type == 10 ? YCGE_REF(REF_GRID, (uint32_t)g.ref) : YCGE_REF(REF_PRIM, prim); }
__global__ __launch_bounds__(256) void k_scene_walk(const GNode *__restrict__ nodes, int n_inner, const uint32_t *__restrict__ leaf_prims, const GPrim *__restrict__ prims,
                                                    GNode *__restrict__ walk)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= 2 * n_inner) return;
    const int i = t >> 1, side = t & 1;
    const GNode src = nodes[i];
    const uint32_t ref = side ? src.rref : src.lref;
    uint32_t out_ref;
    if (YCGE_REF_KIND(ref) == REF_SCENE_NODE) out_ref = YCGE_REF(REF_WALK_NODE, YCGE_REF_PAYLOAD(ref));
    else {
        const uint32_t pay = YCGE_REF_PAYLOAD(ref), start = pay >> 3, count = pay & 7u;
        // the leaf's objects in index order, grids without a solid voxel left out (the first one stays if nothing else does)
        uint32_t obj[7]; int m = 0;
        for (uint32_t k = 0; k < count; k++) {
            const uint32_t pi = leaf_prims[start + k];
            const GPrim &g = prims[pi];
            if (g.type == 10 && g.p[3] < g.p[0]) continue;
            obj[m++] = pi;
        }
        if (m == 0) obj[m++] = leaf_prims[start];
        if (m == 1) out_ref = walk_ref_of(prims[obj[0]], obj[0]);
        else {
            // halve [a, b) until single: the node of a range is created before those of its halves, left half first
            const uint32_t base = (uint32_t)n_inner + (uint32_t)t * YCGE_WALK_LEAF_NODES;
            out_ref = YCGE_REF(REF_WALK_NODE, base | YCGE_WALK_IN_ORDER);
            int ra[8], rb[8], rslot[8], top = 0, next_slot = 1;
            ra[0] = 0; rb[0] = m; rslot[0] = 0; top = 1;
            while (top > 0) {
                top--;
                const int a = ra[top], b = rb[top], slot = rslot[top], mid = a + (b - a + 1) / 2;
                const float inf = __builtin_huge_valf();
                SolidBox L = {{inf, inf, inf}, {-inf, -inf, -inf}}, R = L;
                for (int k = a; k < b; k++) {
                    const SolidBox sb = solid_of(prims[obj[k]]);
                    SolidBox &u = k < mid ? L : R;
                    if (sb.hi[0] < sb.lo[0]) continue;
                    for (int ax = 0; ax < 3; ax++) { u.lo[ax] = fminf(u.lo[ax], sb.lo[ax]); u.hi[ax] = fmaxf(u.hi[ax], sb.hi[ax]); }
                }
                GNode g;
                g.lmin_x = L.lo[0]; g.lmin_y = L.lo[1]; g.lmin_z = L.lo[2]; g.lmax_x = L.hi[0]; g.lmax_y = L.hi[1]; g.lmax_z = L.hi[2];
                g.rmin_x = R.lo[0]; g.rmin_y = R.lo[1]; g.rmin_z = R.lo[2]; g.rmax_x = R.hi[0]; g.rmax_y = R.hi[1]; g.rmax_z = R.hi[2];
                if (mid - a == 1) g.lref = walk_ref_of(prims[obj[a]], obj[a]);
                else { g.lref = YCGE_REF(REF_WALK_NODE, (base + (uint32_t)next_slot) | YCGE_WALK_IN_ORDER); ra[top] = a; rb[top] = mid; rslot[top] = next_slot++; top++; }
                if (b - mid == 1) g.rref = walk_ref_of(prims[obj[mid]], obj[mid]);
                else { g.rref = YCGE_REF(REF_WALK_NODE, (base + (uint32_t)next_slot) | YCGE_WALK_IN_ORDER); ra[top] = mid; rb[top] = b; rslot[top] = next_slot++; top++; }
                g.pad[0] = 0u; g.pad[1] = 0u;
                walk[base + (uint32_t)slot] = g;
            }
        }
    }
    // this side of the scene node's copy: planes and the other reference are written by the two threads of the node between them
    GNode *dst = walk + i;
    if (side == 0) { dst->lmin_x = src.lmin_x; dst->lmin_y = src.lmin_y; dst->lmin_z = src.lmin_z; dst->lmax_z = src.lmax_z; dst->lmax_x = src.lmax_x; dst->lmax_y = src.lmax_y; dst->lref = out_ref; dst->pad[0] = 0u; }
    else { dst->rmin_x = src.rmin_x; dst->rmin_y = src.rmin_y; dst->rmin_z = src.rmin_z; dst->rmax_z = src.rmax_z; dst->rmax_x = src.rmax_x; dst->rmax_y = src.rmax_y; dst->rref = out_ref; dst->pad[1] = 0u; }
}

} // namespace ycge

extern "C" {

// walk: n_inner * (1 + 2 * YCGE_WALK_LEAF_NODES) records of 64 bytes (SceneDev::walk_nodes)
int ycge_launch_scene_walk(const void *nodes, int n_inner, const uint32_t *leaf_prims, const void *prims, void *walk, hipStream_t stream)
{
    if (n_inner <= 0) return 0;
    hipLaunchKernelGGL(ycge::k_scene_walk, dim3((unsigned)((2 * n_inner + 255) / 256)), dim3(256), 0, stream, (const ycge::GNode *)nodes, n_inner, leaf_prims, (const ycge::GPrim *)prims,
                       (ycge::GNode *)walk);
    return (int)hipGetLastError();
}

size_t ycge_bvh_build_scratch_bytes(int n) { return (size_t)(2 * n + 2) * sizeof(ycge::BvhBuildNode); }

// n items (1 .. YCGE_BVH_DEV_MAX_ITEMS); ref_out holds 2 n - 1 records of 40 bytes, gnodes_out n, leaf_out n
int ycge_launch_scene_bvh_build(const float *items, int n, void *scratch, void *ref_out, void *gnodes_out, uint32_t *leaf_out, void *result,
                                int active_waves, hipStream_t stream)
{
    if (n < 1 || n > YCGE_BVH_DEV_MAX_ITEMS) return (int)hipErrorInvalidValue;
    if (active_waves < 1 || active_waves > 16) active_waves = 16;
    static bool lds_set = false;
    if (!lds_set) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(ycge::k_scene_bvh_build), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ycge::BvhShared));
        if (e != hipSuccess) return (int)e;
        lds_set = true;
    }
    hipLaunchKernelGGL(ycge::k_scene_bvh_build, dim3(1), dim3(1024), sizeof(ycge::BvhShared), stream, items, n, (ycge::BvhBuildNode *)scratch, (ycge::RefNodeDev *)ref_out,
                       (ycge::GNode *)gnodes_out, leaf_out, (ycge::BvhBuildResult *)result, active_waves);
    return (int)hipGetLastError();
}


static bool staged_copy_out(void *stage, void *dst, const void *src, size_t bytes)       // device -> page-locked staging -> caller memory (a CPU copy)
{
    if (hipMemcpy(stage, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (size_t i = 0; i < bytes; i++) ((unsigned char *)dst)[i] = ((const unsigned char *)stage)[i];
    return true;
}

// test hook (no context): the kernel on caller-supplied boxes - bounds = n x 6 (min xyz, max xyz), centroids = n x 3.  nodes_out
// holds 2 n records of 40 bytes (reference format, pre-order), leaf_out n, result_out 16 words (BvhBuildResult), build_out (optional)
// 2 n build records of 64 bytes in creation order.  Returns the node count, -1 on a device error, -2 when the kernel fell back.
int ycge_debug_device_bvh(const float *bounds, const float *centroids, int32_t n, void *nodes_out, int32_t *leaf_out, uint32_t *result_out, void *build_out)
{
    if (n < 1 || n > YCGE_BVH_DEV_MAX_ITEMS || !bounds || !centroids || !nodes_out || !leaf_out || !result_out) return -1;
    float *planes = (float *)malloc((size_t)9 * n * sizeof(float));
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) { planes[(size_t)a * n + i] = bounds[6 * i + a]; planes[(size_t)(3 + a) * n + i] = bounds[6 * i + 3 + a]; planes[(size_t)(6 + a) * n + i] = centroids[3 * i + a]; }
    float *d_items = nullptr; void *d_scratch = nullptr, *d_ref = nullptr, *d_g = nullptr, *d_res = nullptr, *stage = nullptr; uint32_t *d_leaf = nullptr;
    int rc = -1;
    struct Out { void *stage; bool operator()(void *dst, const void *src, size_t bytes) const { return staged_copy_out(stage, dst, src, bytes); } } out{nullptr};
    if (hipMalloc((void **)&d_items, (size_t)9 * n * 4) == hipSuccess && hipMalloc(&d_scratch, ycge_bvh_build_scratch_bytes(n)) == hipSuccess &&
        hipMalloc(&d_ref, (size_t)2 * n * 40) == hipSuccess && hipMalloc(&d_g, (size_t)n * 64 + 64) == hipSuccess && hipMalloc(&d_res, 64) == hipSuccess &&
        hipMalloc((void **)&d_leaf, (size_t)n * 4) == hipSuccess && hipMemcpy(d_items, planes, (size_t)9 * n * 4, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemset(d_scratch, 0, ycge_bvh_build_scratch_bytes(n)) == hipSuccess &&
        ycge_launch_scene_bvh_build(d_items, n, d_scratch, d_ref, d_g, d_leaf, d_res, getenv("YCGE_BVH_WAVES") ? atoi(getenv("YCGE_BVH_WAVES")) : 16, nullptr) == 0 && hipDeviceSynchronize() == hipSuccess &&
        hipHostMalloc(&stage, (size_t)2 * n * 64 + 64, hipHostMallocDefault) == hipSuccess && ((out.stage = stage), out(result_out, d_res, 64))) {
        // (every read-back through page-locked staging of this function's own and a CPU copy: the device writes no caller memory - DESIGN section 6)
        const ycge::BvhBuildResult *r = (const ycge::BvhBuildResult *)result_out;
        if (build_out) (void)out(build_out, d_scratch, (size_t)2 * n * 64);
        if (r->fallback) rc = -2;
        else if (out(nodes_out, d_ref, (size_t)r->n_nodes * 40) && out(leaf_out, d_leaf, (size_t)n * 4)) rc = r->n_nodes;
    }
    if (stage) (void)hipHostFree(stage);
    (void)hipFree(d_items); (void)hipFree(d_scratch); (void)hipFree(d_ref); (void)hipFree(d_g); (void)hipFree(d_res); (void)hipFree(d_leaf);
    free(planes);
    return rc;
}

}
