// ycge_bvh_split.hip.h - what the device builders of the two trees share: one wavefront splits one node as the reference's recursive
// builders do (Objects/BVH.cs:258-459 for the scene tree, Objects/MeshBVH.cs:371-576 for a mesh's), and the wavefronts of a workgroup take
// nodes off a queue in LDS.  ycge_bvh_build.hip (scene flavour, one workgroup per tree) and ycge_mesh_bvh_build.hip (mesh flavour, one
// workgroup per subtree) instantiate it; the comment at the top of ycge_bvh_build.hip says why every step gives the reference's result.
// The flavours differ in the leaf size (4 / 8) and in what the partition pass bins with: the scene builder re-derives origin and extent
// from the first and the last item of the range (with a zero guard), the mesh builder keeps the binning bounds (MeshBVH.cs:511-513).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ycge_device.h"
#include "ycge_keysort.h"
#include "ycge_math.h"

namespace ycge {

#define YCGE_BVH_DEV_BINS 16
#define YCGE_BVH_DEV_LEAF 4          // TargetLeafSize, BVH.cs:7
#define YCGE_MESH_BVH_LEAF 8         // MeshBVH.cs:14

struct BvhBuildNode {       // build-time record in global scratch; this workgroup is its only reader and writer
    int32_t start, count, depth, left;      // left < 0: leaf; right = left + 1
    int32_t inner, pre, ipre, pad;          // inner nodes in the subtree; pre-order index over all nodes / over inner nodes
    float mn[3], mx[3];
    int32_t pad2[2];
};
static_assert(sizeof(BvhBuildNode) == 64, "BvhBuildNode");

struct RefNodeDev { float mn[3], mx[3]; int32_t left, right, start, count; };     // = ycge::RefNode (ycge_accel.h)

__device__ __forceinline__ uint32_t fkey(float f) { const uint32_t u = f2u(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float fkey_inv(uint32_t k) { return u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ float box_area(const float mn[3], const float mx[3])
{
    const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
    return 2.0f * (dx * dy + dx * dz + dy * dz);
}

struct BvhWaveBins { uint32_t cnt[3][YCGE_BVH_DEV_BINS]; uint32_t mn[3][YCGE_BVH_DEV_BINS][3], mx[3][YCGE_BVH_DEV_BINS][3]; };

struct BvhShared {
    uint16_t ord[YCGE_BVH_DEV_MAX_ITEMS], ord2[YCGE_BVH_DEV_MAX_ITEMS];
    uint16_t back_l[YCGE_BVH_DEV_MAX_ITEMS];                                        // per node range: the k-th back L, counted from the end (position in the range)
    unsigned long long queue[YCGE_BVH_DEV_MAX_ITEMS];                               // bit 63 valid | depth << 48 | count << 32 | start << 16 | node
    BvhWaveBins bins[16];
    float ikey[YCGE_BVH_DEV_MAX_ITEMS];                                             // Array.Sort case: the sort key of every item of the range, by item
    uint32_t q_head, q_tail, pending, n_nodes, fallback, max_depth, sorts;
};

// the SAH sweep of one node by one wavefront, from the node's bins and the extents of its centroid bounds: the winning (axis, bin), or
// split_bin = -1 and the longest axis when no split is valid
__device__ __forceinline__ void bvh_sah_sweep(const BvhWaveBins &B, const float ext[3], const int lane, int &split_bin, int &best_axis)
{
    // SAH sweep (BVH.cs:354-383), one lane per (axis, bin): lanes 16 a + b.  The running boxes and counts of the reference's two
    // loops are inclusive scans over the 16 bins of an axis - min / max and integer sums, so their grouping is free - and every lane
    // then evaluates the ONE cost expression of its split, larea[b] * lc + rarea[b + 1] * rc, in the reference's operation order.
    // The reference keeps the first strict minimum in (axis, bin) order = the smallest lane among the lanes with the least cost.
    const int sa = lane >> 4, sb = lane & 15;
    const bool slot = lane < 48 && ext[sa < 3 ? sa : 0] > 0.0f;
    int c_pre = 0, c_suf = 0;
    float pmn[3] = {YCGE_INF, YCGE_INF, YCGE_INF}, pmx[3] = {-YCGE_INF, -YCGE_INF, -YCGE_INF};
    if (slot) {
        c_pre = (int)B.cnt[sa][sb];
        if (c_pre > 0)      // an empty bin joins no box (BVH.cs:358, 367)
            for (int k = 0; k < 3; k++) { pmn[k] = fkey_inv(B.mn[sa][sb][k]); pmx[k] = fkey_inv(B.mx[sa][sb][k]); }
    }
    c_suf = c_pre;
    float qmn[3] = {pmn[0], pmn[1], pmn[2]}, qmx[3] = {pmx[0], pmx[1], pmx[2]};
    for (int o = 1; o < 16; o <<= 1) {          // inclusive scans inside the 16-lane segment: prefix from the left, suffix from the right
        const int cu = __shfl_up(c_pre, o, 16), cd = __shfl_down(c_suf, o, 16);
        float umn[3], umx[3], dmn[3], dmx[3];
        for (int k = 0; k < 3; k++) { umn[k] = __shfl_up(pmn[k], o, 16); umx[k] = __shfl_up(pmx[k], o, 16); dmn[k] = __shfl_down(qmn[k], o, 16); dmx[k] = __shfl_down(qmx[k], o, 16); }
        if (sb >= o) { c_pre += cu; for (int k = 0; k < 3; k++) { if (umn[k] < pmn[k]) pmn[k] = umn[k]; if (umx[k] > pmx[k]) pmx[k] = umx[k]; } }
        if (sb + o < 16) { c_suf += cd; for (int k = 0; k < 3; k++) { if (dmn[k] < qmn[k]) qmn[k] = dmn[k]; if (dmx[k] > qmx[k]) qmx[k] = dmx[k]; } }
    }
    // split b: left = bins 0..b (this lane's prefix), right = bins b + 1..15 (the next lane's suffix)
    const int rc = __shfl_down(c_suf, 1, 16);
    float rmn[3], rmx[3];
    for (int k = 0; k < 3; k++) { rmn[k] = __shfl_down(qmn[k], 1, 16); rmx[k] = __shfl_down(qmx[k], 1, 16); }
    float my_cost = YCGE_INF;
    if (slot && sb < 15 && c_pre > 0 && rc > 0) {
        const float cost = box_area(pmn, pmx) * (float)c_pre + box_area(rmn, rmx) * (float)rc;
        if (cost < YCGE_INF) my_cost = cost;            // (+inf and NaN never beat the reference's initial +inf)
    }
    int my_lane = lane;
    for (int o = 32; o > 0; o >>= 1) {
        const float oc = __shfl_xor(my_cost, o, 64);
        const int ol = __shfl_xor(my_lane, o, 64);
        if (oc < my_cost || (oc == my_cost && ol < my_lane)) { my_cost = oc; my_lane = ol; }
    }
    const float best_cost = my_cost;
    split_bin = -1; best_axis = 0;
    if (ext[1] > ext[0] && ext[1] >= ext[2]) best_axis = 1; else if (ext[2] > ext[0] && ext[2] >= ext[1]) best_axis = 2;      // BVH.cs:314-316
    if (best_cost < YCGE_INF) { split_bin = my_lane & 15; best_axis = my_lane >> 4; }
}

// one wavefront splits node `id` = items ord[s .. s + cnt); items: nine planes, n floats apart
template <bool MESH>
__device__ __forceinline__ bool bvh_split_node(BvhShared &sh, const float *__restrict__ items, const int n, BvhBuildNode *__restrict__ nodes, const int id,
                               const int s, const int cnt, const int depth)
{
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    BvhWaveBins &B = sh.bins[wave];
    const float *cpl[3] = {items + (size_t)6 * n, items + (size_t)7 * n, items + (size_t)8 * n};
    // centroid bounds (BVH.cs:300-312)
    float cmn[3] = {YCGE_INF, YCGE_INF, YCGE_INF}, cmx[3] = {-YCGE_INF, -YCGE_INF, -YCGE_INF};
    for (int i = lane; i < cnt; i += 64) {
        const int it = sh.ord[s + i];
        for (int a = 0; a < 3; a++) { const float c = cpl[a][it]; if (c < cmn[a]) cmn[a] = c; if (c > cmx[a]) cmx[a] = c; }
    }
    for (int a = 0; a < 3; a++)
        for (int o = 32; o > 0; o >>= 1) {
            const float lo = __shfl_xor(cmn[a], o, 64), hi = __shfl_xor(cmx[a], o, 64);
            if (lo < cmn[a]) cmn[a] = lo;
            if (hi > cmx[a]) cmx[a] = hi;
        }
    float ext[3], inv_ext[3];
    for (int a = 0; a < 3; a++) { ext[a] = cmx[a] - cmn[a]; inv_ext[a] = 1.0f / ext[a]; }
    // bins of all three axes in one pass over the items
    for (int w = lane; w < 3 * YCGE_BVH_DEV_BINS; w += 64) (&B.cnt[0][0])[w] = 0u;
    for (int w = lane; w < 9 * YCGE_BVH_DEV_BINS; w += 64) { (&B.mn[0][0][0])[w] = 0xffffffffu; (&B.mx[0][0][0])[w] = 0u; }      // min keys start at the top, max keys at the bottom
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < cnt; i += 64) {
        const int it = sh.ord[s + i];
        uint32_t kmn[3], kmx[3];
        for (int k = 0; k < 3; k++) { kmn[k] = fkey(items[(size_t)k * n + it]); kmx[k] = fkey(items[(size_t)(3 + k) * n + it]); }
        for (int a = 0; a < 3; a++) {
            if (!(ext[a] > 0.0f)) continue;
            int b = cs_f2i((cpl[a][it] - cmn[a]) * inv_ext[a] * (float)(YCGE_BVH_DEV_BINS - 1));
            if (b < 0) b = 0;
            if (b >= YCGE_BVH_DEV_BINS) b = YCGE_BVH_DEV_BINS - 1;
            atomicAdd(&B.cnt[a][b], 1u);
            for (int k = 0; k < 3; k++) { atomicMin(&B.mn[a][b][k], kmn[k]); atomicMax(&B.mx[a][b][k], kmx[k]); }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    int split_bin, best_axis;
    bvh_sah_sweep(B, ext, lane, split_bin, best_axis);
    const float *key = cpl[best_axis];
    int mid = 0;
    bool sort_it = split_bin < 0;
    if (!sort_it) {
        // partition (BVH.cs:394-410): bins re-derived from the first and the last item of the range
        // (MeshBVH.cs:511-513: the mesh builder keeps the binning bounds, and has no zero guard - a split exists only on an axis with extent)
        const float origin = MESH ? (best_axis == 0 ? cmn[0] : best_axis == 1 ? cmn[1] : cmn[2]) : key[sh.ord[s]];
        const float extent = key[sh.ord[s + cnt - 1]] - origin;
        const float inv_extent = MESH ? (best_axis == 0 ? inv_ext[0] : best_axis == 1 ? inv_ext[1] : inv_ext[2]) : (extent != 0.0f ? 1.0f / extent : 0.0f);
        const bool zero = !MESH && !(inv_extent != 0.0f);
        auto is_left = [&](int pos) -> bool {
            const int b0 = zero ? 0 : cs_f2i((key[sh.ord[s + pos]] - origin) * inv_extent * (float)(YCGE_BVH_DEV_BINS - 1));
            return b0 <= split_bin;
        };
        int n_left = 0;
        for (int base = 0; base < cnt; base += 64) {
            const int pos = base + lane;
            const bool L = pos < cnt && is_left(pos);
            n_left += __popcll(__ballot(L));
        }
        mid = n_left;
        sort_it = n_left == 0 || n_left == cnt;          // BVH.cs:412-421: a side came out empty - the range is sorted AS THE LOOP LEFT IT
        if (n_left < cnt) {                                // (all left: the loop moved nothing)
            const int e = cnt - 1;
            const int front_hi = mid + (is_left(mid) ? 0 : 1);
            int run_l = 0;
            for (int base = 0; base < cnt; base += 64) {
                const int pos = base + lane;
                const bool in = pos < cnt, L = in && is_left(pos);
                const unsigned long long m = __ballot(L);
                const int pref_l = run_l + __popcll(m & ((1ull << lane) - 1ull));      // L's in [0, pos)
                if (in && pos >= front_hi && L) sh.back_l[s + (n_left - pref_l - 1)] = (uint16_t)pos;     // j - 1 = L's in (pos, e]
                run_l += __popcll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            run_l = 0;
            for (int base = 0; base < cnt; base += 64) {
                const int pos = base + lane;
                const bool in = pos < cnt, L = in && is_left(pos);
                const unsigned long long m = __ballot(L);
                const int pref_l = run_l + __popcll(m & ((1ull << lane) - 1ull));
                if (in) {
                    const uint16_t me = sh.ord[s + pos];
                    if (pos < front_hi) {
                        if (L) sh.ord2[s + pos] = me;
                        else {
                            const int k1 = pos - pref_l;                                    // k - 1 = R's in [0, pos)
                            const int dest = k1 == 0 ? e : (int)sh.back_l[s + k1 - 1] - 1;
                            sh.ord2[s + dest] = me;
                            if (pos < mid) sh.ord2[s + pos] = sh.ord[s + sh.back_l[s + k1]];
                        }
                    } else if (!L) sh.ord2[s + pos - 1] = me;
                }
                run_l += __popcll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < cnt; i += 64) sh.ord[s + i] = sh.ord2[s + i];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (sort_it) {
        // Array.Sort(items, start, count, axis comparer) + median split (BVH.cs:386-391, 414-421).  Every lane runs the same steps
        // on the same slice (one instruction at a time, so reads precede the writes of a step in every lane): no one-lane branch
        for (int i = lane; i < cnt; i += 64) { const int it = sh.ord[s + i]; sh.ikey[it] = key[it]; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        KeySorter<uint16_t> sorter{sh.ord, sh.ikey};
        sorter.sort(s, cnt);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        mid = cnt >> 1;
        if (lane == 0) atomicAdd(&sh.sorts, 1u);
    }
    // children
    int first = 0;
    if (lane == 0) {
        first = (int)atomicAdd(&sh.n_nodes, 2u);
        nodes[id].left = first;
        const int cs[2] = {s, s + mid}, cc[2] = {mid, cnt - mid};
        for (int k = 0; k < 2; k++) {
            BvhBuildNode &c = nodes[first + k];
            c.start = cs[k]; c.count = cc[k]; c.depth = depth + 1; c.left = -1; c.inner = 0; c.pre = 0; c.ipre = 0;
        }
        atomicMax(&sh.max_depth, (uint32_t)(depth + 1));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // the range's new order and the child records before the children are queued
    if (lane == 0) {
        const int cs[2] = {s, s + mid}, cc[2] = {mid, cnt - mid};
        for (int k = 0; k < 2; k++)
            if (cc[k] > (MESH ? YCGE_MESH_BVH_LEAF : YCGE_BVH_DEV_LEAF)) {
                atomicAdd(&sh.pending, 1u);
                const uint32_t slot = atomicAdd(&sh.q_tail, 1u);
                const unsigned long long ent = (1ull << 63) | ((unsigned long long)(depth + 1) << 48) | ((unsigned long long)cc[k] << 32) |
                                               ((unsigned long long)cs[k] << 16) | (unsigned long long)(first + k);
                __hip_atomic_store(&sh.queue[slot], ent, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
    }
    return true;
}

// the workgroup builds the subtrees below the queued nodes: every wavefront takes nodes off the queue until none is left or in flight
template <bool MESH>
__device__ __forceinline__ void bvh_build_loop(BvhShared &sh, const float *__restrict__ items, const int stride, BvhBuildNode *__restrict__ nodes, const int active_waves)
{
    const int tid = (int)threadIdx.x, lane = tid & 63;
    // (lane 0 decides, the decision is broadcast: no loop and no wavefront-wide operation inside a one-lane branch)
    while ((tid >> 6) < active_waves) {
        __builtin_amdgcn_wave_barrier();
        uint32_t got = 0xffffffffu;                 // a queue slot, 0xfffffffe = all done, 0xffffffff = nothing yet
        if (lane == 0) {
            if (__hip_atomic_load(&sh.fallback, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) got = 0xfffffffeu;
            else {
                const uint32_t h = __hip_atomic_load(&sh.q_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (h < __hip_atomic_load(&sh.q_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                    if (atomicCAS(&sh.q_head, h, h + 1u) == h) got = h;
                } else if (__hip_atomic_load(&sh.pending, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) got = 0xfffffffeu;
            }
        }
        got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
        if (got == 0xfffffffeu) break;
        if (got == 0xffffffffu) { __builtin_amdgcn_s_sleep(2); continue; }
        unsigned long long ent;
        do ent = __hip_atomic_load(&sh.queue[got], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); while (!(ent >> 63));       // every lane, one address
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int id = (int)(ent & 0xffffu), s = (int)((ent >> 16) & 0xffffu), cnt = (int)((ent >> 32) & 0xffffu), depth = (int)((ent >> 48) & 0x7fffu);
        const bool ok = depth < 200 && bvh_split_node<MESH>(sh, items, stride, nodes, id, s, cnt, depth);
        if (lane == 0) {
            if (!ok) atomicExch(&sh.fallback, 1u);
            __hip_atomic_fetch_sub(&sh.pending, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

} // namespace ycge
