// ycge_mesh_bvh.cpp - the host side of the device-side mesh BVH build (kernels: ycge_mesh_bvh_build.hip): scratch, the level loop over
// the wide nodes, the read-back of the tree into a BuiltTree - and of the arena assembled on the device behind it (kernels: ycge_mesh_emit.hip).  ycge_scene_upload (ycge_host.cpp)
// picks the builder per mesh, and the two hooks tests and profiles hold the builder by live there too; whatever this builder declines - Array.Sort at a wide node, a non-finite coordinate, a tree
// deeper than the reference accepts - the host builder of ycge_accel.cpp builds, and it is the one that words the errors.
#include "ycge_ctx.h"

namespace ycge_host {

namespace {

enum { MH_N_TOP = 0, MH_N_LEVEL = 1, MH_FALLBACK = 3, MH_N_JOBS = 4, MH_SORTS = 5, MH_MAX_DEPTH = 6, MH_NONFINITE = 7, MH_N_NODES = 8, MH_WORDS = 16 };      // = ycge_mesh_bvh_build.hip

// device -> page-locked staging of the library's own -> host memory, in pieces (the device writes no memory the library does not map)
hipError_t staged_read(PinnedBuf &stage, void *dst, const void *src, size_t bytes, hipStream_t stream)
{
    const size_t piece = (size_t)4 << 20;
    hipError_t e = stage.reserve(bytes < piece ? (bytes > 4096 ? bytes : 4096) : piece);
    for (size_t at = 0; e == hipSuccess && at < bytes; at += stage.bytes) {
        const size_t len = bytes - at < stage.bytes ? bytes - at : stage.bytes;
        e = hipMemcpyAsync(stage.p, (const uint8_t *)src + at, len, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) std::memcpy((uint8_t *)dst + at, stage.p, len);
    }
    return e;
}

} // namespace

int mesh_bvh_build_device(MeshBvhScratch &S, const float *tris9, int32_t n, int wide_min, hipStream_t stream, BuiltTree &out, MeshBvhReport &rep)
{
    out = BuiltTree{};
    rep = MeshBvhReport{};
    if (n <= 0) return YCGE_OK;
    if (wide_min < 9) wide_min = 9;
    if (wide_min > YCGE_BVH_DEV_MAX_ITEMS) wide_min = YCGE_BVH_DEV_MAX_ITEMS;
    const size_t N = (size_t)n;
    const size_t top_bytes = ycge_mesh_bvh_sizes(0), acc_bytes = ycge_mesh_bvh_sizes(1), sub_bytes = ycge_mesh_bvh_sizes(2), scan_block = ycge_mesh_bvh_sizes(3);
    const size_t level_cap = N / (size_t)(wide_min + 1) + 2;                                   // the wide nodes of one level are disjoint ranges of more than wide_min items
    size_t top_cap = 2 * 64 * level_cap + 2;                                                   // 64 levels of them and their children: deeper trees are refused anyway
    if (top_cap > 2 * N + 2) top_cap = 2 * N + 2;
    const size_t n_blk = (N + scan_block - 1) / scan_block;
    auto fail = [&](hipError_t e) { rep.error = e; (void)hipGetLastError(); return e == hipErrorOutOfMemory ? YCGE_ERR_OUT_OF_MEMORY : YCGE_ERR_DEVICE; };
#define MESH_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return fail(e_); } while (0)
    MESH_TRY(S.tris.reserve(9 * N)); MESH_TRY(S.items.reserve(9 * N)); MESH_TRY(S.items_pos.reserve(9 * N));
    MESH_TRY(S.ord.reserve(N)); MESH_TRY(S.ord2.reserve(N)); MESH_TRY(S.lpref.reserve(N)); MESH_TRY(S.back_l.reserve(N)); MESH_TRY(S.leaf.reserve(N));
    MESH_TRY(S.blk.reserve(n_blk + 1)); MESH_TRY(S.blk_excl.reserve(n_blk + 1)); MESH_TRY(S.hdr.reserve(MH_WORDS));
    MESH_TRY(S.node_of.reserve(N)); MESH_TRY(S.level[0].reserve(level_cap)); MESH_TRY(S.level[1].reserve(level_cap)); MESH_TRY(S.jobs.reserve(top_cap));
    MESH_TRY(S.flag.reserve(N)); MESH_TRY(S.top.reserve(top_cap * top_bytes)); MESH_TRY(S.acc.reserve(level_cap * acc_bytes));
    MESH_TRY(S.sub_nodes.reserve(2 * N * sub_bytes)); MESH_TRY(S.nodes.reserve(2 * N * sizeof(RefNode)));
    MESH_TRY(hipMemcpyAsync(S.tris.p, tris9, 9 * N * sizeof(float), hipMemcpyHostToDevice, stream));
    MESH_TRY(hipMemsetAsync(S.hdr.p, 0, MH_WORDS * 4, stream));
    MESH_TRY(hipStreamSynchronize(stream));
    const auto t0 = std::chrono::steady_clock::now();
    auto launched = [&](int e) { return (hipError_t)e; };
    uint32_t hdr[MH_WORDS];
    const int wide = n > wide_min ? 1 : 0;
    MESH_TRY(launched(ycge_launch_mesh_items(S.tris.p, n, S.items.p, S.hdr.p, stream)));
    MESH_TRY(launched(ycge_launch_mesh_init(n, wide, S.ord.p, S.node_of.p, S.top.p, S.level[0].p, S.jobs.p, S.hdr.p, stream)));
    int n_cur = wide, level = 0;
    MESH_TRY(staged_read(S.stage, hdr, S.hdr.p, sizeof hdr, stream));
    if (hdr[MH_NONFINITE]) { rep.fallback = MESH_BVH_NON_FINITE; return 1; }       // before any kernel bins a NaN
    while (n_cur > 0) {
        if (level >= 64) { rep.fallback = MESH_BVH_TOO_DEEP; return 1; }
        const int next_slot = (level + 1) & 1;
        MESH_TRY(launched(ycge_launch_mesh_wide_level(S.items.p, n, n_cur, wide_min, next_slot, S.ord.p, S.ord2.p, S.node_of.p, S.level[level & 1].p, S.level[next_slot].p,
                                                      S.jobs.p, S.top.p, (int)top_cap, S.acc.p, S.flag.p, S.lpref.p, S.blk.p, S.blk_excl.p, S.back_l.p, S.hdr.p, stream)));
        MESH_TRY(staged_read(S.stage, hdr, S.hdr.p, sizeof hdr, stream));
        rep.wide_nodes += n_cur;
        rep.levels = ++level;
        if (hdr[MH_FALLBACK]) { rep.fallback = (int)hdr[MH_FALLBACK]; return 1; }
        n_cur = (int)hdr[MH_N_LEVEL + next_slot];
    }
    const int n_jobs = (int)hdr[MH_N_JOBS], n_top = (int)hdr[MH_N_TOP];
    rep.jobs = n_jobs;
    MESH_TRY(launched(ycge_launch_mesh_subtrees(S.items.p, n, S.ord.p, S.items_pos.p, S.jobs.p, n_jobs, S.top.p, S.sub_nodes.p, S.leaf.p, S.hdr.p, stream)));
    MESH_TRY(staged_read(S.stage, hdr, S.hdr.p, sizeof hdr, stream));
    if (hdr[MH_FALLBACK]) { rep.fallback = (int)hdr[MH_FALLBACK]; return 1; }
    MESH_TRY(launched(ycge_launch_mesh_assemble(S.top.p, n_top, level, S.jobs.p, n_jobs, S.sub_nodes.p, S.nodes.p, S.hdr.p, stream)));
    MESH_TRY(staged_read(S.stage, hdr, S.hdr.p, sizeof hdr, stream));
    const size_t n_nodes = hdr[MH_N_NODES];
    if (n_nodes < 1 || n_nodes > 2 * N) return fail(hipErrorUnknown);
    out.nodes.resize(n_nodes);
    out.leaf_index.resize(N);
    MESH_TRY(staged_read(S.stage, out.nodes.data(), S.nodes.p, n_nodes * sizeof(RefNode), stream));
    MESH_TRY(staged_read(S.stage, out.leaf_index.data(), S.leaf.p, N * 4, stream));
#undef MESH_TRY
    out.root = 0;
    out.max_depth = (int32_t)hdr[MH_MAX_DEPTH];
    out.sort_fallbacks = (int32_t)hdr[MH_SORTS];
    rep.us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return YCGE_OK;
}

// ---- the arena on the device (ycge_mesh_emit.hip) ----------------------------------------------------------------------------------

namespace {
enum { EH_UNITS = 0, EH_MESH0 = 4, EH_MESH_WORDS = 4 };      // = ycge_mesh_emit.hip
}

uint32_t mesh_arena_treelet_offset(size_t rec_bytes, bool any_root_is_a_node, size_t &total_bytes)
{
    const size_t n_units = rec_bytes / 32;
    const size_t t0 = (rec_bytes + 511) & ~(size_t)511;
    const size_t total = t0 + n_units * YCGE_TL_BYTES_PER_UNIT;
    total_bytes = rec_bytes;
    if (n_units == 0 || total + 4096 >= (1ull << 32) || !any_root_is_a_node) return 0;
    total_bytes = total;
    return (uint32_t)t0;
}

hipError_t mesh_emit_add(MeshEmit &E, size_t mi, bool built, MeshBvhScratch &S, const BuiltTree &t, const float *tris9, int32_t n_tris, const int32_t *tri_material, int32_t material)
{
    if (E.in.size() <= mi) E.in.resize(mi + 1);
    MeshEmit::Input &I = E.in[mi];
    I.ready = true;
    I.material = material;
    I.n_nodes = (uint32_t)t.nodes.size();
    I.n_tris = n_tris > 0 ? (uint32_t)n_tris : 0u;
    if (t.root < 0 || I.n_nodes == 0 || I.n_tris == 0) { I.n_nodes = 0; return hipSuccess; }
    I.root_count = t.nodes[0].count > 0 ? t.nodes[0].count : 0;
    const size_t N = I.n_tris;
    hipError_t e = hipSuccess;
    if (built) { I.tris = std::move(S.tris); I.nodes = std::move(S.nodes); I.leaf = std::move(S.leaf); }       // (the next build reserves its own)
    else {
        if ((e = I.tris.reserve(9 * N)) != hipSuccess || (e = I.nodes.reserve((size_t)I.n_nodes * sizeof(RefNode))) != hipSuccess || (e = I.leaf.reserve(N)) != hipSuccess) return e;
        if ((e = hipMemcpy(I.tris.p, tris9, 9 * N * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(I.nodes.p, t.nodes.data(), (size_t)I.n_nodes * sizeof(RefNode), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(I.leaf.p, t.leaf_index.data(), N * 4, hipMemcpyHostToDevice)) != hipSuccess) return e;
    }
    if (tri_material) {
        if ((e = I.tri_material.reserve(N)) != hipSuccess) return e;
        e = hipMemcpy(I.tri_material.p, tri_material, N * 4, hipMemcpyHostToDevice);
    }
    return e;
}

hipError_t mesh_emit_layout(MeshEmit &E, PinnedBuf &stage, hipStream_t stream)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n_hdr = EH_MESH0 + EH_MESH_WORDS * E.in.size();
    uint64_t n_refs = 0;
    uint32_t max_nodes = 1;
    for (MeshEmit::Input &I : E.in) {
        I.first_ref = (uint32_t)n_refs;
        n_refs += I.n_nodes;
        if (I.n_nodes > max_nodes) max_nodes = I.n_nodes;
    }
    if (n_refs > 0x0fffffffu) return hipErrorInvalidValue;          // (2^28 nodes: their records are far past the arena's 2^25 units)
    E.n_refs = (uint32_t)n_refs;
    hipError_t e = hipSuccess;
    if ((e = E.refs.reserve(n_refs ? n_refs : 1)) != hipSuccess || (e = E.tiles.reserve(ycge_launch_mesh_emit_tiles(max_nodes))) != hipSuccess || (e = E.hdr.reserve(n_hdr)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(E.hdr.p, 0, n_hdr * 4, stream)) != hipSuccess) return e;
    for (size_t mi = 0; mi < E.in.size(); mi++) {
        const MeshEmit::Input &I = E.in[mi];
        if (I.n_nodes == 0) continue;
        if ((e = (hipError_t)ycge_launch_mesh_emit_layout(I.nodes.p, I.n_nodes, (uint32_t)mi, E.tiles.p, E.refs.p + I.first_ref, E.hdr.p, stream)) != hipSuccess) return e;
    }
    E.hdr_host.assign(n_hdr, 0u);
    e = staged_read(stage, E.hdr_host.data(), E.hdr.p, n_hdr * 4, stream);
    E.us[0] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return e;
}

hipError_t mesh_emit_write(MeshEmit &E, uint8_t *arena, uint32_t rec_units, size_t total_bytes, uint32_t tl_offset, int32_t n_materials, bool timed, PinnedBuf &stage, hipStream_t stream)
{
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](double &us) { const auto t1 = std::chrono::steady_clock::now(); us = std::chrono::duration<double, std::micro>(t1 - t0).count(); t0 = t1; };
    const size_t rec_bytes = (size_t)rec_units * 32, n_hdr = EH_MESH0 + EH_MESH_WORDS * E.in.size();
    hipError_t e = hipSuccess;
    if (total_bytes > rec_bytes && (e = hipMemsetAsync(arena + rec_bytes, 0, total_bytes - rec_bytes, stream)) != hipSuccess) return e;
    for (size_t mi = 0; mi < E.in.size(); mi++) {
        const MeshEmit::Input &I = E.in[mi];
        if (I.n_nodes == 0) continue;
        e = (hipError_t)ycge_launch_mesh_emit_records(I.nodes.p, I.n_nodes, I.n_tris, (uint32_t)mi, E.refs.p + I.first_ref, I.leaf.p, I.tris.p, I.tri_material.p, I.material, n_materials,
                                                      arena, rec_units, E.hdr.p, stream);
        if (e != hipSuccess) return e;
    }
    if (timed) { if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e; lap(E.us[1]); }
    if (tl_offset != 0 && E.n_refs != 0 && (e = (hipError_t)ycge_launch_mesh_emit_treelets(E.refs.p, E.n_refs, arena, tl_offset, stream)) != hipSuccess) return e;
    E.hdr_host.assign(n_hdr, 0u);
    e = staged_read(stage, E.hdr_host.data(), E.hdr.p, n_hdr * 4, stream);
    lap(E.us[timed ? 2 : 1]);
    if (!timed) E.us[2] = 0.0;
    return e;
}

} // namespace ycge_host
