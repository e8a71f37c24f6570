// ycge_mesh_bvh.cpp - the host side of the device-side mesh BVH build (kernels: ycge_mesh_bvh_build.hip): scratch, the level loop over
// the wide nodes, the read-back of the tree into a BuiltTree.  ycge_scene_upload (ycge_host.cpp)
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

} // namespace ycge_host
