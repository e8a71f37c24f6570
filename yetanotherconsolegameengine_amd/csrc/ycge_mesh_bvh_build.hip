// ycge_mesh_bvh_build.hip - a mesh's triangle BVH (Objects/MeshBVH.cs:371-576, triangle bounds :340-363) built ON THE DEVICE at
// ycge_scene_upload: the tree build_tree(items, TreeFlavour::Mesh) of ycge_accel.cpp returns, byte for byte - that host builder is the
// sequential statement of the same thing and what the tests compare this against.  ycge_bvh_build.hip does it for the scene tree inside
// one workgroup (at most YCGE_BVH_DEV_MAX_ITEMS items in LDS); a mesh has no such ceiling, so the tree is built in four parts:
//   1. k_mesh_items: triangle_items' arithmetic per triangle, nine planes (box min, box max, centroid), and a flag for anything non-finite;
//   2. the WIDE nodes - more items than one workgroup holds - are split level by level, all wide nodes of a level in the same launches,
//      over ONE item order in global memory (`ord`, positions 0 .. n; a node is a range of positions, node_of[position] names the wide
//      node of the level the position lies in).  Centroid bounds and the bins of all three axes are min / max / integer sums on
//      order-preserving keys (order-free: per-workgroup in LDS where a workgroup's positions lie in one node, merged by global atomics);
//      one wavefront per node runs the SAH sweep (bvh_sah_sweep, the code the one-workgroup builders run); the partition is the closed
//      form of the reference's two-pointer loop (top of ycge_bvh_build.hip, tests/test_partition_closed_form.py): a prefix count of the
//      L items - one scan over all positions, a node's counts are differences of it - the list of its back L's, a scatter into `ord2`.
//      A wide node that needs Array.Sort (no valid split, or a side came out empty) is not built here: `fallback`, the host builds the mesh;
//   3. every node at or below the one-workgroup capacity is a JOB: one workgroup of k_mesh_subtrees builds the whole subtree below it
//      with the queue-of-nodes code of ycge_bvh_split.hip.h in the mesh flavour, on the items gathered into position order;
//   4. assembly: subtree sizes bottom-up over the wide nodes, pre-order numbers top-down, inner boxes with MathF.Min / Max; a job's nodes
//      follow its root.  A leaf's `start` is its first position: the leaves in pre-order cover the positions in ascending order.
// The host side (ycge_mesh_bvh.cpp) drives the levels and reads the tree back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ycge_bvh_split.hip.h"

namespace ycge {

struct MeshTopNode {        // a node made by the wide path, in creation order
    int32_t start, count, depth, left;          // left < 0: a job (k_mesh_subtrees); else the children are left, left + 1
    int32_t size, pre, level_index, mid;        // nodes in the subtree; pre-order number; index in its level's list (-1: a job); items of the left child
    float mn[3], mx[3];
    int32_t pad[2];
};
static_assert(sizeof(MeshTopNode) == 64, "MeshTopNode");

struct MeshWideAcc {        // what the launches of one level hand on about one wide node
    BvhWaveBins bins;
    uint32_t cmn[3], cmx[3];                    // centroid bounds, as keys
    float origin, inv_extent;                   // the partition's bin parameters (MeshBVH.cs:511-513)
    int32_t split_bin, axis;
    uint32_t pad[2];
};

// (MH_FALLBACK keeps the FIRST reason given: a node without a split is named by the sweep, before its empty side is seen)
enum { MH_N_TOP = 0, MH_N_LEVEL = 1 /* and 2: the levels take them in turn */, MH_FALLBACK = 3, MH_N_JOBS = 4, MH_SORTS = 5, MH_MAX_DEPTH = 6, MH_NONFINITE = 7, MH_N_NODES = 8 };
#define YCGE_MESH_SCAN_BLOCK 1024       // positions per workgroup of the flag / prefix pass
#define YCGE_MESH_BIN_BLOCK 1024        // positions per workgroup of the bounds / bins passes (256 threads, 4 each)

// L items in positions [0, pos): the in-workgroup prefix plus the scanned workgroup totals (pos = n: the total)
__device__ __forceinline__ uint32_t mesh_pref(const uint32_t *__restrict__ lpref, const uint32_t *__restrict__ blk_excl, int pos, int n)
{
    return pos >= n ? blk_excl[(n + YCGE_MESH_SCAN_BLOCK - 1) / YCGE_MESH_SCAN_BLOCK] : lpref[pos] + blk_excl[pos / YCGE_MESH_SCAN_BLOCK];
}

// ---------------------------------------------------------------------------------- 1. items
__global__ __launch_bounds__(256) void k_mesh_items(const float *__restrict__ t9, const int n, float *__restrict__ items, uint32_t *__restrict__ hdr)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const float *t = t9 + (size_t)9 * i;
    const float eps = 1e-4f;        // MeshBVH.cs:351
    bool finite = true;
    for (int a = 0; a < 3; a++) {
        const float A = t[a], B = t[3 + a], C = t[6 + a];
        const float mn = cs_min(A, cs_min(B, C)) - eps;
        const float mx = cs_max(A, cs_max(B, C)) + eps;
        const float c = 0.5f * (mn + mx);
        items[(size_t)a * n + i] = mn; items[(size_t)(3 + a) * n + i] = mx; items[(size_t)(6 + a) * n + i] = c;
        finite = finite && cs_isfinite(A) && cs_isfinite(B) && cs_isfinite(C) && cs_isfinite(mn) && cs_isfinite(mx) && cs_isfinite(c);
    }
    if (!finite) atomicOr(&hdr[MH_NONFINITE], 1u);
}

__global__ __launch_bounds__(256) void k_mesh_init(const int n, const int wide, uint32_t *__restrict__ ord, int32_t *__restrict__ node_of, MeshTopNode *__restrict__ top,
                                                   int32_t *__restrict__ level0, int32_t *__restrict__ jobs, uint32_t *__restrict__ hdr)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < n) { ord[i] = (uint32_t)i; node_of[i] = wide ? 0 : -1; }
    if (i == 0) {
        MeshTopNode &r = top[0];
        r.start = 0; r.count = n; r.depth = 1; r.left = -1; r.size = 0; r.pre = 0; r.level_index = wide ? 0 : -1; r.mid = 0;
        hdr[MH_N_TOP] = 1u; hdr[MH_N_LEVEL] = wide ? 1u : 0u; hdr[MH_N_LEVEL + 1] = 0u; hdr[MH_FALLBACK] = 0u; hdr[MH_N_JOBS] = wide ? 0u : 1u;
        hdr[MH_SORTS] = 0u; hdr[MH_MAX_DEPTH] = 1u; hdr[MH_N_NODES] = 0u;
        if (wide) level0[0] = 0; else jobs[0] = 0;
    }
}

// ---------------------------------------------------------------------------------- 2. wide nodes, one level
__global__ __launch_bounds__(256) void k_wide_reset(MeshWideAcc *__restrict__ acc, const int n_cur, uint32_t *__restrict__ hdr, const int next_slot)
{
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t == 0) hdr[MH_N_LEVEL + next_slot] = 0u;
    const int words = (int)(sizeof(MeshWideAcc) / 4), li = t / words, w = t % words;
    if (li >= n_cur) return;
    uint32_t v = 0u;        // counts, max keys: from the bottom
    const int cnt_words = 3 * YCGE_BVH_DEV_BINS, box_words = 9 * YCGE_BVH_DEV_BINS;
    if ((w >= cnt_words && w < cnt_words + box_words) || (w >= cnt_words + 2 * box_words && w < cnt_words + 2 * box_words + 3)) v = 0xffffffffu;      // min keys: from the top
    ((uint32_t *)&acc[li])[w] = v;
}

// does the workgroup's range of positions lie in ONE wide node?  A node is a range of positions, so two ends in the same node decide;
// two ends in no wide node decide nothing (a wide node may lie between them): -2, every position is looked at on its own
__device__ __forceinline__ int mesh_block_node(const int32_t *__restrict__ node_of, int base, int n)
{
    const int last = base + YCGE_MESH_BIN_BLOCK - 1 < n - 1 ? base + YCGE_MESH_BIN_BLOCK - 1 : n - 1;
    const int a = node_of[base], b = node_of[last];
    return a >= 0 && a == b ? a : -2;
}

__global__ __launch_bounds__(256) void k_wide_bounds(const float *__restrict__ items, const int n, const uint32_t *__restrict__ ord, const int32_t *__restrict__ node_of,
                                                     MeshWideAcc *__restrict__ acc)
{
    __shared__ uint32_t s_mn[3], s_mx[3];
    const int tid = (int)threadIdx.x, base = (int)blockIdx.x * YCGE_MESH_BIN_BLOCK;
    const int one = mesh_block_node(node_of, base, n);
    if (tid < 3) { s_mn[tid] = 0xffffffffu; s_mx[tid] = 0u; }
    __syncthreads();
    for (int j = 0; j < YCGE_MESH_BIN_BLOCK / 256; j++) {
        const int pos = base + j * 256 + tid;
        if (pos >= n) break;
        const int li = one >= 0 ? one : node_of[pos];
        if (li < 0) continue;
        const uint32_t it = ord[pos];
        for (int a = 0; a < 3; a++) {
            const uint32_t k = fkey(items[(size_t)(6 + a) * n + it]);
            if (one >= 0) { atomicMin(&s_mn[a], k); atomicMax(&s_mx[a], k); }
            else { atomicMin(&acc[li].cmn[a], k); atomicMax(&acc[li].cmx[a], k); }
        }
    }
    if (one < 0) return;
    __syncthreads();
    if (tid < 3) { atomicMin(&acc[one].cmn[tid], s_mn[tid]); atomicMax(&acc[one].cmx[tid], s_mx[tid]); }
}

__global__ __launch_bounds__(256) void k_wide_bins(const float *__restrict__ items, const int n, const uint32_t *__restrict__ ord, const int32_t *__restrict__ node_of,
                                                   MeshWideAcc *__restrict__ acc)
{
    __shared__ BvhWaveBins s_bins;
    const int tid = (int)threadIdx.x, base = (int)blockIdx.x * YCGE_MESH_BIN_BLOCK;
    const int one = mesh_block_node(node_of, base, n);
    for (int w = tid; w < 3 * YCGE_BVH_DEV_BINS; w += 256) (&s_bins.cnt[0][0])[w] = 0u;
    for (int w = tid; w < 9 * YCGE_BVH_DEV_BINS; w += 256) { (&s_bins.mn[0][0][0])[w] = 0xffffffffu; (&s_bins.mx[0][0][0])[w] = 0u; }
    __syncthreads();
    for (int j = 0; j < YCGE_MESH_BIN_BLOCK / 256; j++) {
        const int pos = base + j * 256 + tid;
        if (pos >= n) break;
        const int li = one >= 0 ? one : node_of[pos];
        if (li < 0) continue;
        MeshWideAcc &A = acc[li];
        BvhWaveBins &B = one >= 0 ? s_bins : A.bins;
        const uint32_t it = ord[pos];
        uint32_t kmn[3], kmx[3];
        for (int k = 0; k < 3; k++) { kmn[k] = fkey(items[(size_t)k * n + it]); kmx[k] = fkey(items[(size_t)(3 + k) * n + it]); }
        for (int a = 0; a < 3; a++) {
            const float cmn = fkey_inv(A.cmn[a]), ext = fkey_inv(A.cmx[a]) - cmn;
            if (!(ext > 0.0f)) continue;
            const float inv_ext = 1.0f / ext;
            int b = cs_f2i((items[(size_t)(6 + a) * n + it] - cmn) * inv_ext * (float)(YCGE_BVH_DEV_BINS - 1));
            if (b < 0) b = 0;
            if (b >= YCGE_BVH_DEV_BINS) b = YCGE_BVH_DEV_BINS - 1;
            atomicAdd(&B.cnt[a][b], 1u);
            for (int k = 0; k < 3; k++) { atomicMin(&B.mn[a][b][k], kmn[k]); atomicMax(&B.mx[a][b][k], kmx[k]); }
        }
    }
    if (one < 0) return;
    __syncthreads();
    BvhWaveBins &G = acc[one].bins;
    for (int w = tid; w < 3 * YCGE_BVH_DEV_BINS; w += 256) { const uint32_t v = (&s_bins.cnt[0][0])[w]; if (v) atomicAdd(&(&G.cnt[0][0])[w], v); }
    for (int w = tid; w < 9 * YCGE_BVH_DEV_BINS; w += 256) {
        const uint32_t lo = (&s_bins.mn[0][0][0])[w], hi = (&s_bins.mx[0][0][0])[w];
        if (lo != 0xffffffffu) atomicMin(&(&G.mn[0][0][0])[w], lo);
        if (hi != 0u) atomicMax(&(&G.mx[0][0][0])[w], hi);
    }
}

// one wavefront per wide node
__global__ __launch_bounds__(64) void k_wide_sweep(MeshWideAcc *__restrict__ acc, const int n_cur, uint32_t *__restrict__ hdr)
{
    const int li = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (li >= n_cur) return;
    MeshWideAcc &A = acc[li];
    float cmn[3], ext[3];
    for (int a = 0; a < 3; a++) { cmn[a] = fkey_inv(A.cmn[a]); ext[a] = fkey_inv(A.cmx[a]) - cmn[a]; }
    int split_bin, best_axis;
    bvh_sah_sweep(A.bins, ext, lane, split_bin, best_axis);
    if (lane == 0) {
        A.split_bin = split_bin; A.axis = best_axis;
        A.origin = best_axis == 0 ? cmn[0] : best_axis == 1 ? cmn[1] : cmn[2];
        A.inv_extent = 1.0f / (best_axis == 0 ? ext[0] : best_axis == 1 ? ext[1] : ext[2]);
        if (split_bin < 0) atomicCAS(&hdr[MH_FALLBACK], 0u, 1u);        // Array.Sort at a wide node
    }
}

// which side every position of a wide node goes to, its count of L's before it inside the workgroup, the workgroup's total
__global__ __launch_bounds__(YCGE_MESH_SCAN_BLOCK) void k_wide_flags(const float *__restrict__ items, const int n, const uint32_t *__restrict__ ord,
                                                                    const int32_t *__restrict__ node_of, const MeshWideAcc *__restrict__ acc,
                                                                    uint8_t *__restrict__ flag, uint32_t *__restrict__ lpref, uint32_t *__restrict__ blk)
{
    __shared__ uint32_t s_wave[YCGE_MESH_SCAN_BLOCK / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, pos = (int)blockIdx.x * YCGE_MESH_SCAN_BLOCK + tid;
    bool L = false;
    if (pos < n) {
        const int li = node_of[pos];
        if (li >= 0 && acc[li].split_bin >= 0) {
            const MeshWideAcc &A = acc[li];
            const float key = items[(size_t)(6 + A.axis) * n + ord[pos]];
            L = cs_f2i((key - A.origin) * A.inv_extent * (float)(YCGE_BVH_DEV_BINS - 1)) <= A.split_bin;
        }
    }
    const unsigned long long m = __ballot(L);
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u, total = 0u;
    for (int w = 0; w < YCGE_MESH_SCAN_BLOCK / 64; w++) { const uint32_t v = s_wave[w]; if (w < wave) before += v; total += v; }
    if (pos < n) { flag[pos] = L ? 1 : 0; lpref[pos] = before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); }
    if (tid == 0) blk[blockIdx.x] = total;
}

// exclusive scan of the workgroup totals, one workgroup; blk_excl[n_blk] = the total
__global__ __launch_bounds__(1024) void k_mesh_scan_blocks(const uint32_t *__restrict__ blk, uint32_t *__restrict__ blk_excl, const int n_blk)
{
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_run;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_run = 0u;
    __syncthreads();
    for (int base = 0; base < n_blk; base += 1024) {
        const int i = base + tid;
        const uint32_t v = i < n_blk ? blk[i] : 0u;
        uint32_t inc = v;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t before = s_run, total = 0u;
        for (int w = 0; w < 16; w++) { const uint32_t u = s_wave[w]; if (w < wave) before += u; total += u; }
        if (i < n_blk) blk_excl[i] = before + inc - v;
        __syncthreads();
        if (tid == 0) s_run += total;
        __syncthreads();
    }
    if (tid == 0) blk_excl[n_blk] = s_run;
}

struct MeshRange { int s, cnt, n_left, rel, pref_l, front_hi; bool L, live; };
// a position's place in the partition of its wide node (live: the node has a split with both sides taken)
__device__ __forceinline__ MeshRange mesh_range(const int pos, const int n, const int32_t *__restrict__ node_of, const int32_t *__restrict__ level,
                                                const MeshTopNode *__restrict__ top, const uint8_t *__restrict__ flag, const uint32_t *__restrict__ lpref,
                                                const uint32_t *__restrict__ blk_excl)
{
    MeshRange r;
    r.live = false;
    if (pos >= n) return r;
    const int li = node_of[pos];
    if (li < 0) return r;
    const MeshTopNode &nd = top[level[li]];
    r.s = nd.start; r.cnt = nd.count;
    const uint32_t p0 = mesh_pref(lpref, blk_excl, r.s, n);
    r.n_left = (int)(mesh_pref(lpref, blk_excl, r.s + r.cnt, n) - p0);
    if (r.n_left == 0 || r.n_left == r.cnt) return r;
    r.rel = pos - r.s;
    r.pref_l = (int)(lpref[pos] + blk_excl[pos / YCGE_MESH_SCAN_BLOCK] - p0);
    r.L = flag[pos] != 0;
    r.front_hi = r.n_left + (flag[r.s + r.n_left] ? 0 : 1);
    r.live = true;
    return r;
}

// the back L's of every wide node, counted from the end of its range
__global__ __launch_bounds__(256) void k_wide_back_l(const int n, const int32_t *__restrict__ node_of, const int32_t *__restrict__ level, const MeshTopNode *__restrict__ top,
                                                     const uint8_t *__restrict__ flag, const uint32_t *__restrict__ lpref, const uint32_t *__restrict__ blk_excl,
                                                     uint32_t *__restrict__ back_l)
{
    const int pos = (int)(blockIdx.x * 256u + threadIdx.x);
    const MeshRange r = mesh_range(pos, n, node_of, level, top, flag, lpref, blk_excl);
    if (!r.live) return;
    if (r.rel >= r.front_hi && r.L) back_l[r.s + (r.n_left - r.pref_l - 1)] = (uint32_t)r.rel;       // j - 1 = L's in (pos, e]
}

// every item of a wide node to the slot the two-pointer loop leaves it in (the closed form, top of ycge_bvh_build.hip)
__global__ __launch_bounds__(256) void k_wide_scatter(const int n, const int32_t *__restrict__ node_of, const int32_t *__restrict__ level, const MeshTopNode *__restrict__ top,
                                                      const uint8_t *__restrict__ flag, const uint32_t *__restrict__ lpref, const uint32_t *__restrict__ blk_excl,
                                                      const uint32_t *__restrict__ back_l, const uint32_t *__restrict__ ord, uint32_t *__restrict__ ord2)
{
    const int pos = (int)(blockIdx.x * 256u + threadIdx.x);
    const MeshRange r = mesh_range(pos, n, node_of, level, top, flag, lpref, blk_excl);
    if (!r.live) return;
    const uint32_t me = ord[pos];
    const int mid = r.n_left, e = r.cnt - 1;
    if (r.rel < r.front_hi) {
        if (r.L) ord2[pos] = me;
        else {
            const int k1 = r.rel - r.pref_l;                                            // k - 1 = R's in [0, pos)
            const int dest = k1 == 0 ? e : (int)back_l[r.s + k1 - 1] - 1;
            ord2[r.s + dest] = me;
            if (r.rel < mid) ord2[pos] = ord[r.s + (int)back_l[r.s + k1]];
        }
    } else if (!r.L) ord2[pos - 1] = me;
}

// the two children of every wide node of the level: wide ones join the next level's list, the others the jobs
__global__ __launch_bounds__(256) void k_wide_children(const int n, const int n_cur, const int32_t *__restrict__ level, MeshTopNode *__restrict__ top, const int top_cap,
                                                       const uint32_t *__restrict__ lpref, const uint32_t *__restrict__ blk_excl, int32_t *__restrict__ level_next,
                                                       int32_t *__restrict__ jobs, uint32_t *__restrict__ hdr, const int wide_min, const int next_slot)
{
    const int li = (int)(blockIdx.x * 256u + threadIdx.x);
    if (li >= n_cur) return;
    MeshTopNode &nd = top[level[li]];
    const int s = nd.start, cnt = nd.count;
    const int n_left = (int)(mesh_pref(lpref, blk_excl, s + cnt, n) - mesh_pref(lpref, blk_excl, s, n));
    if (n_left == 0 || n_left == cnt) { atomicCAS(&hdr[MH_FALLBACK], 0u, 2u); return; }       // a side came out empty: Array.Sort at a wide node
    const int first = (int)atomicAdd(&hdr[MH_N_TOP], 2u);
    if (first + 2 > top_cap) { atomicCAS(&hdr[MH_FALLBACK], 0u, 3u); return; }
    const int cs[2] = {s, s + n_left}, cc[2] = {n_left, cnt - n_left};
    for (int k = 0; k < 2; k++) {
        MeshTopNode &c = top[first + k];
        c.start = cs[k]; c.count = cc[k]; c.depth = nd.depth + 1; c.left = -1; c.size = 0; c.pre = 0; c.mid = 0;
        if (cc[k] > wide_min) { const int slot = (int)atomicAdd(&hdr[MH_N_LEVEL + next_slot], 1u); level_next[slot] = first + k; c.level_index = slot; }
        else { const int slot = (int)atomicAdd(&hdr[MH_N_JOBS], 1u); jobs[slot] = first + k; c.level_index = -1; }
    }
    nd.mid = n_left;
    nd.left = first;
}

// the new order of the level's ranges, and the wide node of the next level every position lies in
__global__ __launch_bounds__(256) void k_wide_commit(const int n, int32_t *__restrict__ node_of, const int32_t *__restrict__ level, const MeshTopNode *__restrict__ top,
                                                     uint32_t *__restrict__ ord, const uint32_t *__restrict__ ord2)
{
    const int pos = (int)(blockIdx.x * 256u + threadIdx.x);
    if (pos >= n) return;
    const int li = node_of[pos];
    if (li < 0) return;
    const MeshTopNode &nd = top[level[li]];
    if (nd.left < 0) { node_of[pos] = -1; return; }       // (not split: the build has fallen back)
    ord[pos] = ord2[pos];
    node_of[pos] = top[nd.left + (pos < nd.start + nd.mid ? 0 : 1)].level_index;
}

// ---------------------------------------------------------------------------------- 3. subtrees
__global__ __launch_bounds__(256) void k_mesh_gather(const float *__restrict__ items, const int n, const uint32_t *__restrict__ ord, float *__restrict__ items_pos)
{
    const int pos = (int)(blockIdx.x * 256u + threadIdx.x);
    if (pos >= n) return;
    const uint32_t it = ord[pos];
    for (int p = 0; p < 9; p++) items_pos[(size_t)p * n + pos] = items[(size_t)p * n + it];
}

// one workgroup per job: the subtree below a node of at most YCGE_BVH_DEV_MAX_ITEMS items, as k_scene_bvh_build builds the scene tree -
// items_pos: the nine planes in position order, so a job's items are 0 .. count of its own slice; nodes: 2 records per position
__global__ __launch_bounds__(1024) void k_mesh_subtrees(const float *__restrict__ items_pos, const int n, const uint32_t *__restrict__ ord, const int32_t *__restrict__ jobs,
                                                        MeshTopNode *__restrict__ top, BvhBuildNode *__restrict__ sub_nodes, uint32_t *__restrict__ leaf_out,
                                                        uint32_t *__restrict__ hdr)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char bvh_lds[];
    BvhShared &sh = *reinterpret_cast<BvhShared *>(bvh_lds);
    const int tid = (int)threadIdx.x;
    MeshTopNode &J = top[jobs[blockIdx.x]];
    const int s = J.start, cnt = J.count, d0 = J.depth;
    const float *items = items_pos + s;
    BvhBuildNode *nodes = sub_nodes + (size_t)2 * s;
    for (int i = tid; i < cnt; i += 1024) { sh.ord[i] = (uint16_t)i; sh.queue[i] = 0ull; }
    if (tid == 0) {
        sh.q_head = 0; sh.q_tail = 0; sh.pending = 0; sh.n_nodes = 1; sh.fallback = 0; sh.max_depth = (uint32_t)d0; sh.sorts = 0;
        BvhBuildNode &r = nodes[0];
        r.start = 0; r.count = cnt; r.depth = d0; r.left = -1; r.inner = 0; r.pre = 0; r.ipre = 0;
    }
    __syncthreads();
    if (tid == 0 && cnt > YCGE_MESH_BVH_LEAF) {
        sh.pending = 1; sh.q_tail = 1;
        sh.queue[0] = (1ull << 63) | ((unsigned long long)d0 << 48) | ((unsigned long long)cnt << 32);
    }
    __syncthreads();
    int waves = (cnt + 63) / 64;
    if (waves > 16) waves = 16;
    bvh_build_loop<true>(sh, items, n, nodes, waves);
    __syncthreads();
    const int n_nodes = (int)sh.n_nodes, max_depth = (int)sh.max_depth;
    if (sh.fallback) { if (tid == 0) atomicCAS(&hdr[MH_FALLBACK], 0u, 4u); return; }       // deeper than any tree the reference accepts
    // leaf boxes: one lane, compare-assign in leaf order (MeshBVH.cs leaf bounds; the sign of a zero is the first item's)
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
    for (int d = max_depth - 1; d >= d0; d--) {
        for (int i = tid; i < n_nodes; i += 1024) {
            BvhBuildNode &nd = nodes[i];
            if (nd.left < 0 || nd.depth != d) continue;
            const BvhBuildNode &L = nodes[nd.left], &R = nodes[nd.left + 1];
            for (int k = 0; k < 3; k++) { nd.mn[k] = cs_min(L.mn[k], R.mn[k]); nd.mx[k] = cs_max(L.mx[k], R.mx[k]); }      // MathF.Min / Max
            nd.inner = 1 + L.inner + R.inner;
        }
        __syncthreads();
    }
    for (int d = d0; d < max_depth; d++) {
        for (int i = tid; i < n_nodes; i += 1024) {
            BvhBuildNode &nd = nodes[i];
            if (nd.left < 0 || nd.depth != d) continue;
            BvhBuildNode &L = nodes[nd.left], &R = nodes[nd.left + 1];
            L.pre = nd.pre + 1;
            R.pre = nd.pre + 1 + 2 * L.inner + 1;
        }
        __syncthreads();
    }
    for (int i = tid; i < cnt; i += 1024) leaf_out[s + i] = ord[s + sh.ord[i]];
    if (tid == 0) {
        J.size = n_nodes;
        for (int k = 0; k < 3; k++) { J.mn[k] = nodes[0].mn[k]; J.mx[k] = nodes[0].mx[k]; }
        if (sh.sorts) atomicAdd(&hdr[MH_SORTS], sh.sorts);
        atomicMax(&hdr[MH_MAX_DEPTH], (uint32_t)max_depth);
    }
}

// ---------------------------------------------------------------------------------- 4. assembly
// one workgroup: sizes and boxes of the wide nodes bottom-up, pre-order numbers top-down, their records
__global__ __launch_bounds__(1024) void k_mesh_assemble(MeshTopNode *__restrict__ top, const int n_top, const int n_levels, RefNodeDev *__restrict__ out, uint32_t *__restrict__ hdr)
{
    const int tid = (int)threadIdx.x;
    for (int d = n_levels; d >= 1; d--) {
        for (int i = tid; i < n_top; i += 1024) {
            MeshTopNode &nd = top[i];
            if (nd.left < 0 || nd.depth != d) continue;
            const MeshTopNode &L = top[nd.left], &R = top[nd.left + 1];
            for (int k = 0; k < 3; k++) { nd.mn[k] = cs_min(L.mn[k], R.mn[k]); nd.mx[k] = cs_max(L.mx[k], R.mx[k]); }
            nd.size = 1 + L.size + R.size;
        }
        __syncthreads();
    }
    for (int d = 1; d <= n_levels; d++) {
        for (int i = tid; i < n_top; i += 1024) {
            const MeshTopNode &nd = top[i];
            if (nd.left < 0 || nd.depth != d) continue;
            MeshTopNode &L = top[nd.left], &R = top[nd.left + 1];
            L.pre = nd.pre + 1;
            R.pre = nd.pre + 1 + L.size;
        }
        __syncthreads();
    }
    for (int i = tid; i < n_top; i += 1024) {
        const MeshTopNode &nd = top[i];
        if (nd.left < 0) continue;
        RefNodeDev o;
        for (int k = 0; k < 3; k++) { o.mn[k] = nd.mn[k]; o.mx[k] = nd.mx[k]; }
        o.left = top[nd.left].pre; o.right = top[nd.left + 1].pre; o.start = 0; o.count = 0;
        out[nd.pre] = o;
    }
    if (tid == 0) hdr[MH_N_NODES] = (uint32_t)top[0].size;
}

// one workgroup per job: its nodes behind its root's pre-order number
__global__ __launch_bounds__(256) void k_mesh_emit(const MeshTopNode *__restrict__ top, const int32_t *__restrict__ jobs, const BvhBuildNode *__restrict__ sub_nodes,
                                                   RefNodeDev *__restrict__ out)
{
    const MeshTopNode &J = top[jobs[blockIdx.x]];
    const BvhBuildNode *nodes = sub_nodes + (size_t)2 * J.start;
    for (int i = (int)threadIdx.x; i < J.size; i += 256) {
        const BvhBuildNode &nd = nodes[i];
        RefNodeDev o;
        for (int k = 0; k < 3; k++) { o.mn[k] = nd.mn[k]; o.mx[k] = nd.mx[k]; }
        if (nd.left < 0) { o.left = o.right = -1; o.start = J.start + nd.start; o.count = nd.count; }
        else { o.left = J.pre + nodes[nd.left].pre; o.right = J.pre + nodes[nd.left + 1].pre; o.start = 0; o.count = 0; }
        out[J.pre + nd.pre] = o;
    }
}

} // namespace ycge

extern "C" {

using namespace ycge;

size_t ycge_mesh_bvh_sizes(int which)
{
    switch (which) {
    case 0: return sizeof(MeshTopNode);
    case 1: return sizeof(MeshWideAcc);
    case 2: return sizeof(BvhBuildNode);
    case 3: return YCGE_MESH_SCAN_BLOCK;
    }
    return 0;
}

static unsigned blocks_of(int n, int per) { return (unsigned)((n + per - 1) / per); }

// tris9 -> the nine item planes; hdr (16 words, zeroed by the caller) gets the non-finite flag
int ycge_launch_mesh_items(const float *tris9, int n, float *items, uint32_t *hdr, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mesh_items, dim3(blocks_of(n, 256)), dim3(256), 0, stream, tris9, n, items, hdr);
    return (int)hipGetLastError();
}

int ycge_launch_mesh_init(int n, int wide, uint32_t *ord, int32_t *node_of, void *top, int32_t *level0, int32_t *jobs, uint32_t *hdr, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mesh_init, dim3(blocks_of(n, 256)), dim3(256), 0, stream, n, wide, ord, node_of, (MeshTopNode *)top, level0, jobs, hdr);
    return (int)hipGetLastError();
}

// one level of wide nodes: `level` lists its n_cur nodes, level_next / hdr[MH_N_LEVEL + next_slot] receive the next level's
int ycge_launch_mesh_wide_level(const float *items, int n, int n_cur, int wide_min, int next_slot, uint32_t *ord, uint32_t *ord2, int32_t *node_of, const int32_t *level,
                                int32_t *level_next, int32_t *jobs, void *top, int top_cap, void *acc, uint8_t *flag, uint32_t *lpref, uint32_t *blk, uint32_t *blk_excl,
                                uint32_t *back_l, uint32_t *hdr, hipStream_t stream)
{
    MeshTopNode *T = (MeshTopNode *)top;
    MeshWideAcc *A = (MeshWideAcc *)acc;
    const unsigned per_pos = blocks_of(n, 256), n_blk = blocks_of(n, YCGE_MESH_SCAN_BLOCK);
    hipLaunchKernelGGL(k_wide_reset, dim3(blocks_of(n_cur * (int)(sizeof(MeshWideAcc) / 4), 256)), dim3(256), 0, stream, A, n_cur, hdr, next_slot);
    hipLaunchKernelGGL(k_wide_bounds, dim3(blocks_of(n, YCGE_MESH_BIN_BLOCK)), dim3(256), 0, stream, items, n, ord, node_of, A);
    hipLaunchKernelGGL(k_wide_bins, dim3(blocks_of(n, YCGE_MESH_BIN_BLOCK)), dim3(256), 0, stream, items, n, ord, node_of, A);
    hipLaunchKernelGGL(k_wide_sweep, dim3((unsigned)n_cur), dim3(64), 0, stream, A, n_cur, hdr);
    hipLaunchKernelGGL(k_wide_flags, dim3(n_blk), dim3(YCGE_MESH_SCAN_BLOCK), 0, stream, items, n, ord, node_of, A, flag, lpref, blk);
    hipLaunchKernelGGL(k_mesh_scan_blocks, dim3(1), dim3(1024), 0, stream, blk, blk_excl, (int)n_blk);
    hipLaunchKernelGGL(k_wide_back_l, dim3(per_pos), dim3(256), 0, stream, n, node_of, level, T, flag, lpref, blk_excl, back_l);
    hipLaunchKernelGGL(k_wide_scatter, dim3(per_pos), dim3(256), 0, stream, n, node_of, level, T, flag, lpref, blk_excl, back_l, ord, ord2);
    hipLaunchKernelGGL(k_wide_children, dim3(blocks_of(n_cur, 256)), dim3(256), 0, stream, n, n_cur, level, T, top_cap, lpref, blk_excl, level_next, jobs, hdr, wide_min, next_slot);
    hipLaunchKernelGGL(k_wide_commit, dim3(per_pos), dim3(256), 0, stream, n, node_of, level, T, ord, ord2);
    return (int)hipGetLastError();
}

// the items into position order, then every job's subtree, one workgroup each
int ycge_launch_mesh_subtrees(const float *items, int n, const uint32_t *ord, float *items_pos, const int32_t *jobs, int n_jobs, void *top, void *sub_nodes,
                              uint32_t *leaf_out, uint32_t *hdr, hipStream_t stream)
{
    static bool lds_set = false;
    if (!lds_set) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_mesh_subtrees), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(BvhShared));
        if (e != hipSuccess) return (int)e;
        lds_set = true;
    }
    hipLaunchKernelGGL(k_mesh_gather, dim3(blocks_of(n, 256)), dim3(256), 0, stream, items, n, ord, items_pos);
    hipLaunchKernelGGL(k_mesh_subtrees, dim3((unsigned)n_jobs), dim3(1024), sizeof(BvhShared), stream, items_pos, n, ord, jobs, (MeshTopNode *)top, (BvhBuildNode *)sub_nodes,
                       leaf_out, hdr);
    return (int)hipGetLastError();
}

// nodes_out: the reference-format records in pre-order (2 n of 40 bytes at most); hdr[MH_N_NODES] = how many
int ycge_launch_mesh_assemble(void *top, int n_top, int n_levels, const int32_t *jobs, int n_jobs, const void *sub_nodes, void *nodes_out, uint32_t *hdr, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mesh_assemble, dim3(1), dim3(1024), 0, stream, (MeshTopNode *)top, n_top, n_levels, (RefNodeDev *)nodes_out, hdr);
    hipLaunchKernelGGL(k_mesh_emit, dim3((unsigned)n_jobs), dim3(256), 0, stream, (const MeshTopNode *)top, jobs, (const BvhBuildNode *)sub_nodes, (RefNodeDev *)nodes_out);
    return (int)hipGetLastError();
}

}
