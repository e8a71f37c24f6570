// ycge_mesh_emit.hip - a mesh's device records and the cooperative walk's treelets, written on the device (host side: ycge_mesh_bvh.cpp).
//
// The host's emit_mesh_records (ycge_mesh_bvh.cpp) is a depth-first recursion over a tree whose nodes are numbered in pre-order, left
// before right: the record of node i lies behind the records of the nodes 0 .. i - 1.  With a record's size in 32-byte units - 2 for an
// internal node (GNode), 3 * ((count + 1) / 2) for a leaf (GTriPair records) - a node's unit is the arena's units before the mesh plus the
// exclusive prefix sum of the sizes, and every record is a function of its own node, its two children and the leaf's triangles.  Per mesh,
// reduce-then-scan over tiles as ycge_ansi.hip does it:
//   k_emit_count    per tile of kEmitTile nodes: its units
//   k_emit_scan     one workgroup: the tiles' first units behind the meshes before (the running total lives in hdr), the mesh's units
//   k_emit_layout   per tile: the sizes again, a workgroup scan, every node's REFERENCE (kind, unit, count) as its parent will hold it
//   k_emit_records  a lane per node: the GNode from the children's boxes and references, or the leaf's pair records
// and once, over the nodes of all meshes, behind every mesh's records
//   k_emit_treelets a lane per slot: the 14 GTreeSlots of every internal node, each from the GNode of its parent slot
// append_treelets fills a zeroed region; so does the host side here (hipMemsetAsync), the kernel writes the valid slots only.
// Its own translation unit: the code objects of the frame kernels stay what they were.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ycge_device.h"

namespace {

using namespace ycge;

constexpr int kEmitBlock = 256;
constexpr int kEmitPerLane = 4;                                   // consecutive nodes per lane
constexpr int kEmitTile = kEmitBlock * kEmitPerLane;

struct RefNodeDev { float mn[3], mx[3]; int32_t left, right, start, count; };     // = ycge::RefNode (ycge_accel.h)
static_assert(sizeof(RefNodeDev) == 40, "RefNodeDev");

// hdr: [0] the units of the meshes laid out so far (saturating), then four words per mesh
enum { EH_UNITS = 0, EH_MESH0 = 4, EH_MESH_UNITS = 0, EH_MESH_BAD_LEAF = 1, EH_MESH_BAD_MATERIAL = 2, EH_MESH_WORDS = 4 };      // = ycge_mesh_bvh.cpp

// a leaf above 15 triangles has no record (emit_mesh_records appends nothing and the upload is refused)
__device__ __forceinline__ uint32_t node_units(int32_t count) { return count <= 0 ? 2u : count > 15 ? 0u : 3u * (((uint32_t)count + 1u) >> 1); }

// the units of this lane's kEmitPerLane nodes (a lane past the end counts 0)
__device__ __forceinline__ uint32_t lane_units(const RefNodeDev *__restrict__ nodes, uint32_t n, uint32_t first, int32_t *count)
{
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kEmitPerLane; k++) {
        count[k] = first + k < n ? nodes[first + k].count : -1;
        sum += first + k < n ? node_units(count[k]) : 0u;
    }
    return sum;
}

// exclusive scan of one value per lane over the workgroup (wave prefix by __shfl_up, the wave totals through LDS); total: the sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wsum, uint32_t &total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kEmitBlock / 64; w++) {
        const uint32_t s = wsum[w];
        before += w < wid ? s : 0u;
        total += s;
    }
    __syncthreads();                      // (wsum may be reused)
    return before + inc - v;
}

__global__ __launch_bounds__(kEmitBlock) void k_emit_count(const RefNodeDev *__restrict__ nodes, uint32_t n, uint32_t *__restrict__ tile_units)
{
    __shared__ uint32_t wsum[kEmitBlock / 64];
    int32_t count[kEmitPerLane];
    const uint32_t mine = lane_units(nodes, n, blockIdx.x * (uint32_t)kEmitTile + threadIdx.x * (uint32_t)kEmitPerLane, count);
    uint32_t total;
    (void)block_exclusive_scan(mine, wsum, total);
    if (threadIdx.x == 0) tile_units[blockIdx.x] = total;
}

// one workgroup: tile_units -> the tiles' first units in place, behind the hdr[EH_UNITS] units of the meshes before; the mesh's own units
__global__ __launch_bounds__(kEmitBlock) void k_emit_scan(uint32_t *__restrict__ tiles, uint32_t n_tiles, uint32_t *__restrict__ hdr, uint32_t mesh)
{
    __shared__ uint32_t wsum[kEmitBlock / 64];
    const uint32_t base = hdr[EH_UNITS];
    unsigned long long carry = 0;          // (a mesh's units may pass 2^32 before the host refuses them at 2^25)
    for (uint32_t at = 0; at < n_tiles; at += kEmitBlock) {
        const uint32_t t = at + threadIdx.x;
        const uint32_t v = t < n_tiles ? tiles[t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, wsum, total);
        if (t < n_tiles) tiles[t] = base + (uint32_t)carry + ex;
        carry += total;
    }
    __syncthreads();                       // every lane has read hdr[EH_UNITS]
    if (threadIdx.x == 0) {
        const unsigned long long all = (unsigned long long)base + carry;
        hdr[EH_MESH0 + EH_MESH_WORDS * mesh + EH_MESH_UNITS] = carry > 0xffffffffull ? 0xffffffffu : (uint32_t)carry;
        hdr[EH_UNITS] = all > 0xffffffffull ? 0xffffffffu : (uint32_t)all;
    }
}

__global__ __launch_bounds__(kEmitBlock) void k_emit_layout(const RefNodeDev *__restrict__ nodes, uint32_t n, const uint32_t *__restrict__ tile_first,
                                                            uint32_t *__restrict__ refs, uint32_t *__restrict__ hdr_mesh)
{
    __shared__ uint32_t wsum[kEmitBlock / 64];
    int32_t count[kEmitPerLane];
    const uint32_t first = blockIdx.x * (uint32_t)kEmitTile + threadIdx.x * (uint32_t)kEmitPerLane;
    const uint32_t mine = lane_units(nodes, n, first, count);
    uint32_t total;
    uint32_t unit = tile_first[blockIdx.x] + block_exclusive_scan(mine, wsum, total);
    bool bad = false;
#pragma unroll
    for (int k = 0; k < kEmitPerLane; k++) {
        if (first + k >= n) continue;
        const int32_t c = count[k];
        uint32_t ref = YCGE_REF(REF_MESH_NODE, unit << 4);
        if (c > 15) { ref = YCGE_REF_NONE_VALUE; bad = true; }
        else if (c > 0) ref = YCGE_REF(REF_MESH_LEAF, (unit << 4) | (uint32_t)c);
        refs[first + k] = ref;
        unit += node_units(c);
    }
    if (bad) atomicOr(&hdr_mesh[EH_MESH_BAD_LEAF], 1u);
}

struct TriSlot { float a[3], e1[3], e2[3]; int32_t orig, material; };

// one slot of a pair record as emit_mesh_records computes it (MeshBVH.cs:87-91): three subtractions per edge
__device__ __forceinline__ TriSlot tri_slot(const float *__restrict__ tris9, const int32_t *__restrict__ tri_material, int32_t material, int32_t n_materials,
                                            uint32_t n_tris, uint32_t ti, bool &bad_material)
{
    if (ti >= n_tris) ti = 0;
    const float *v = tris9 + 9 * (size_t)ti;
    TriSlot s;
    s.a[0] = v[0]; s.a[1] = v[1]; s.a[2] = v[2];
    s.e1[0] = v[3] - v[0]; s.e1[1] = v[4] - v[1]; s.e1[2] = v[5] - v[2];
    s.e2[0] = v[6] - v[0]; s.e2[1] = v[7] - v[1]; s.e2[2] = v[8] - v[2];
    s.orig = (int32_t)ti;
    s.material = tri_material ? tri_material[ti] : material;
    if (s.material < 0 || s.material >= n_materials) bad_material = true;
    return s;
}

struct EmitMesh {
    const RefNodeDev *nodes;
    const uint32_t *refs;                 // per node, k_emit_layout
    const uint32_t *leaf;                 // leafTriIndex
    const float *tris9;
    const int32_t *tri_material;          // null: `material` for every triangle
    uint32_t n, n_tris;
    int32_t material, n_materials;
};

// A lane per node, every byte of its records in 16-byte stores (the padding and an odd leaf's empty slot are zeros, as on the host).
// arena_units: the arena's size - a reference past it (only a refused layout holds one) writes nothing.
__global__ __launch_bounds__(kEmitBlock) void k_emit_records(EmitMesh m, uint8_t *__restrict__ arena, uint32_t arena_units, uint32_t *__restrict__ hdr_mesh)
{
    const uint32_t i = blockIdx.x * (uint32_t)kEmitBlock + threadIdx.x;
    if (i >= m.n) return;
    const RefNodeDev &nd = m.nodes[i];
    const uint32_t ref = m.refs[i];
    if (ref == YCGE_REF_NONE_VALUE) return;
    const uint32_t unit = (ref & 0x1ffffff0u) >> 4;
    const int32_t count = nd.count;
    if (unit + node_units(count) > arena_units) return;
    float4 *out = reinterpret_cast<float4 *>(arena + (size_t)unit * 32u);
    if (count <= 0) {
        if ((uint32_t)nd.left >= m.n || (uint32_t)nd.right >= m.n) return;          // (no tree of the builders: nothing is read out of bounds)
        const RefNodeDev &L = m.nodes[nd.left], &R = m.nodes[nd.right];
        out[0] = make_float4(L.mn[0], L.mn[1], L.mn[2], L.mx[2]);
        out[1] = make_float4(L.mx[0], L.mx[1], R.mn[0], R.mn[1]);
        out[2] = make_float4(R.mn[2], R.mx[2], R.mx[0], R.mx[1]);
        out[3] = make_float4(__uint_as_float(m.refs[nd.left]), __uint_as_float(m.refs[nd.right]), 0.0f, 0.0f);
        return;
    }
    if (nd.start < 0 || (uint32_t)nd.start + (uint32_t)count > m.n_tris) return;
    bool bad_material = false;
    const uint32_t *li = m.leaf + nd.start;
    for (int32_t k = 0; k < count; k += 2, out += 6) {
        const TriSlot s0 = tri_slot(m.tris9, m.tri_material, m.material, m.n_materials, m.n_tris, li[k], bad_material);
        TriSlot s1 = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0, 0};
        if (k + 1 < count) s1 = tri_slot(m.tris9, m.tri_material, m.material, m.n_materials, m.n_tris, li[k + 1], bad_material);
        out[0] = make_float4(s0.a[0], s1.a[0], s0.a[1], s1.a[1]);
        out[1] = make_float4(s0.a[2], s1.a[2], s0.e1[0], s1.e1[0]);
        out[2] = make_float4(s0.e1[1], s1.e1[1], s0.e1[2], s1.e1[2]);
        out[3] = make_float4(s0.e2[0], s1.e2[0], s0.e2[1], s1.e2[1]);
        out[4] = make_float4(s0.e2[2], s1.e2[2], __int_as_float(s0.orig), __int_as_float(s1.orig));
        out[5] = make_float4(__int_as_float(s0.material), __int_as_float(s1.material), 0.0f, 0.0f);
    }
    if (bad_material) atomicOr(&hdr_mesh[EH_MESH_BAD_MATERIAL], 1u);
}

__device__ __forceinline__ bool is_mesh_node(uint32_t ref) { return YCGE_REF_KIND(ref) == REF_MESH_NODE; }
__device__ __forceinline__ const GNode *node_at(const uint8_t *arena, uint32_t ref) { return reinterpret_cast<const GNode *>(arena + (size_t)((ref & 0x1ffffff0u) >> 4) * 32u); }

// Sixteen lanes per node of `refs` (the references of all meshes' nodes, one array), lane s < 14 its slot s: slots 2b + 2 / 2b + 3 are the
// children of the node in slot b (b = -1: the node itself), down to depth 3 while the parent slot holds a REF_MESH_NODE (append_treelets).
// A slot is its parent's GNode read again - one or two dependent reads below the node's own - so nothing is carried between nodes.
__global__ __launch_bounds__(kEmitBlock) void k_emit_treelets(const uint32_t *__restrict__ refs, uint32_t n, uint8_t *__restrict__ arena, uint32_t tl_offset)
{
    const uint32_t t = blockIdx.x * (uint32_t)kEmitBlock + threadIdx.x;
    const uint32_t i = t >> 4, s = t & 15u;
    if (i >= n || s >= (uint32_t)YCGE_TL_SLOTS) return;
    const uint32_t ref = refs[i];
    if (!is_mesh_node(ref)) return;                                   // (REF_NONE is kind 7)
    // the chain of parent slots from the node down to slot s: at most two steps
    const uint32_t b1 = s >= 2u ? (s - 2u) >> 1 : 0u;                 // parent slot of s (s >= 2)
    const uint32_t b2 = b1 >= 2u ? (b1 - 2u) >> 1 : 0u;               // ... and its parent (s >= 6)
    const GNode *g = node_at(arena, ref);
    if (s >= 6u) {
        const uint32_t r = (b2 & 1u) ? g->rref : g->lref;
        if (!is_mesh_node(r)) return;
        g = node_at(arena, r);
    }
    if (s >= 2u) {
        const uint32_t r = (b1 & 1u) ? g->rref : g->lref;
        if (!is_mesh_node(r)) return;
        g = node_at(arena, r);
    }
    const float4 q0 = reinterpret_cast<const float4 *>(g)[0], q1 = reinterpret_cast<const float4 *>(g)[1], q2 = reinterpret_cast<const float4 *>(g)[2];
    float4 o0, o1;
    if (s & 1u) {          // right child: rmin xyz, rmax xyz
        o0 = make_float4(q1.z, q1.w, q2.x, q2.z);
        o1 = make_float4(q2.w, q2.y, __uint_as_float(g->rref), __uint_as_float(1u));
    } else {               // left child
        o0 = make_float4(q0.x, q0.y, q0.z, q1.x);
        o1 = make_float4(q1.y, q0.w, __uint_as_float(g->lref), __uint_as_float(1u));
    }
    float4 *out = reinterpret_cast<float4 *>(arena + (size_t)tl_offset + (size_t)((ref & 0x1ffffff0u) >> 4) * YCGE_TL_BYTES_PER_UNIT + (size_t)s * sizeof(GTreeSlot));
    out[0] = o0;
    out[1] = o1;
}

unsigned blocks_of(uint32_t n, uint32_t per) { return (unsigned)((n + per - 1u) / per); }

} // namespace

// the tiles of a mesh of n nodes: the length of the tile array ycge_launch_mesh_emit_layout is given
extern "C" uint32_t ycge_launch_mesh_emit_tiles(uint32_t n_nodes) { return (n_nodes + (uint32_t)kEmitTile - 1u) / (uint32_t)kEmitTile; }

// The layout of mesh number `mesh` (n_nodes >= 1 pre-order records of 40 bytes) behind the meshes laid out before it on `stream`:
// refs[i] = the reference of node i (REF_NONE for a leaf above 15 triangles).  hdr: 4 + 4 * meshes words, zeroed before the first mesh of
// an upload; [0] the arena's units so far, [4 + 4 mesh ..] = {the mesh's units, a leaf above 15 triangles, a material out of range
// (k_emit_records), 0}.  Three launches.
extern "C" int ycge_launch_mesh_emit_layout(const void *nodes, uint32_t n_nodes, uint32_t mesh, uint32_t *tiles, uint32_t *refs, uint32_t *hdr, hipStream_t stream)
{
    if (!nodes || !tiles || !refs || !hdr || n_nodes == 0 || n_nodes > 0x7fffffffu) return (int)hipErrorInvalidValue;
    const uint32_t n_tiles = ycge_launch_mesh_emit_tiles(n_nodes);
    const RefNodeDev *N = static_cast<const RefNodeDev *>(nodes);
    hipLaunchKernelGGL(k_emit_count, dim3(n_tiles), dim3(kEmitBlock), 0, stream, N, n_nodes, tiles);
    hipLaunchKernelGGL(k_emit_scan, dim3(1), dim3(kEmitBlock), 0, stream, tiles, n_tiles, hdr, mesh);
    hipLaunchKernelGGL(k_emit_layout, dim3(n_tiles), dim3(kEmitBlock), 0, stream, N, n_nodes, (const uint32_t *)tiles, refs, hdr + EH_MESH0 + EH_MESH_WORDS * mesh);
    return (int)hipGetLastError();
}

// the records of that mesh into the arena of arena_units units (leaf: n_tris indices, tris9: n_tris * 9, tri_material: n_tris or null)
extern "C" int ycge_launch_mesh_emit_records(const void *nodes, uint32_t n_nodes, uint32_t n_tris, uint32_t mesh, const uint32_t *refs, const uint32_t *leaf, const float *tris9,
                                             const int32_t *tri_material, int32_t material, int32_t n_materials, uint8_t *arena, uint32_t arena_units, uint32_t *hdr,
                                             hipStream_t stream)
{
    if (!nodes || !refs || !leaf || !tris9 || !arena || !hdr || n_nodes == 0 || n_nodes > 0x7fffffffu || n_tris == 0) return (int)hipErrorInvalidValue;
    EmitMesh m;
    m.nodes = static_cast<const RefNodeDev *>(nodes); m.refs = refs; m.leaf = leaf; m.tris9 = tris9; m.tri_material = tri_material;
    m.n = n_nodes; m.n_tris = n_tris; m.material = material; m.n_materials = n_materials;
    hipLaunchKernelGGL(k_emit_records, dim3(blocks_of(n_nodes, kEmitBlock)), dim3(kEmitBlock), 0, stream, m, arena, arena_units, hdr + EH_MESH0 + EH_MESH_WORDS * mesh);
    return (int)hipGetLastError();
}

// the treelets of every internal node among the n_nodes references of all meshes, into the zeroed region at tl_offset (one launch)
extern "C" int ycge_launch_mesh_emit_treelets(const uint32_t *refs, uint32_t n_nodes, uint8_t *arena, uint32_t tl_offset, hipStream_t stream)
{
    if (!refs || !arena || n_nodes == 0 || n_nodes > 0x0fffffffu || tl_offset == 0 || (tl_offset & 511u)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_emit_treelets, dim3(blocks_of(n_nodes * 16u, kEmitBlock)), dim3(kEmitBlock), 0, stream, refs, n_nodes, arena, tl_offset);
    return (int)hipGetLastError();
}
