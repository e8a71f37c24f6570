// ycge_mesh_bvh.cpp - the host side of the device-side mesh BVH build (kernels: ycge_mesh_bvh_build.hip): scratch, the level loop over
// the wide nodes, the read-back of the tree into a BuiltTree - and of the arena assembled on the device behind it (kernels: ycge_mesh_emit.hip),
// with the host's emit beside it (emit_mesh_records, append_treelets).  build_mesh_tree is the choice of builder ycge_scene_upload
// (ycge_scene.cpp) makes per mesh: whatever the device builder declines - Array.Sort at a wide node, a non-finite coordinate, a tree deeper
// than the reference accepts - the host builder of ycge_accel.cpp builds, and it is the one that words the errors.  The hooks tests and
// profiles hold the builders and the two emits by live at the end of the file.
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

// YCGE_OK: `out` is the host builder's tree of tris9, byte for byte; 1: not built, rep.fallback says why; YCGE_ERR_*: rep.error
static int mesh_bvh_build_device(MeshBvhScratch &S, const float *tris9, int32_t n, int wide_min, hipStream_t stream, BuiltTree &out, MeshBvhReport &rep, bool tris_on_device = false)
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
    MESH_TRY(hipMemcpyAsync(S.tris.p, tris9, 9 * N * sizeof(float), tris_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
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

// the host builder (MeshBVH ctor, MeshBVH.cs:41-130; ycge_accel.cpp)
static void host_mesh_tree(const float *tris9, int32_t n, BuiltTree &t)
{
    BoundsSoA items;
    triangle_items(tris9, n, items);
    build_tree(items, TreeFlavour::Mesh, t);
}

int build_mesh_tree(const Knobs &knobs, bool always_try_device, MeshBvhScratch &S, const float *tris9, int32_t n, hipStream_t stream, BuiltTree &t, bool &on_device, MeshBvhReport &rep,
                    const float *d_tris9)
{
    rep = MeshBvhReport{};
    on_device = always_try_device || (!knobs.mesh_bvh_host && n >= 1 && n >= knobs.mesh_bvh_device_min);
    if (on_device) {
        const int rc = mesh_bvh_build_device(S, d_tris9 ? d_tris9 : tris9, n, knobs.mesh_bvh_wide_min, stream, t, rep, d_tris9 != nullptr);
        if (rc < 0) return rc;
        on_device = rc == YCGE_OK;
    }
    if (!on_device && !tris9 && n > 0) return 1;          // (a soup that lives on the device alone: the caller reads it back and asks again)
    if (!on_device) host_mesh_tree(tris9, n, t);
    return YCGE_OK;
}

// a tree into a hook's arrays (nodes_out: 2 n records of 40 bytes, leaf_out: n, stats_out: {root, depth, Array.Sort cases} or null); the node count
static int tree_out(const BuiltTree &t, void *nodes_out, int32_t *leaf_out, int32_t *stats_out)
{
    if (!t.nodes.empty()) std::memcpy(nodes_out, t.nodes.data(), t.nodes.size() * sizeof(RefNode));
    if (!t.leaf_index.empty()) std::memcpy(leaf_out, t.leaf_index.data(), t.leaf_index.size() * 4);
    if (stats_out) { stats_out[0] = t.root; stats_out[1] = t.max_depth; stats_out[2] = t.sort_fallbacks; }
    return (int)t.nodes.size();
}

// ---- the arena on the device (ycge_mesh_emit.hip) ----------------------------------------------------------------------------------

namespace {
enum { EH_UNITS = 0, EH_MESH0 = 4, EH_MESH_WORDS = 4 };      // = ycge_mesh_emit.hip
}

// where the treelet region of an arena of rec_bytes of records starts (0: none, append_treelets' conditions) and where the arena then ends
static uint32_t mesh_arena_treelet_offset(size_t rec_bytes, bool any_root_is_a_node, size_t &total_bytes)
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

// every mesh's layout; hdr_host on return (stage: the builder's page-locked staging).  base_units == null: the meshes lie one behind the
// other from unit 0 (an upload); else mesh mi lies from unit base_units[mi] on (a pooled arena: the header's unit count is preset to it)
static hipError_t mesh_emit_layout(MeshEmit &E, PinnedBuf &stage, hipStream_t stream, const uint32_t *base_units = nullptr)
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
        if (base_units && (e = hipMemsetD32Async((hipDeviceptr_t)(E.hdr.p + EH_UNITS), (int)base_units[mi], 1, stream)) != hipSuccess) return e;
        if ((e = (hipError_t)ycge_launch_mesh_emit_layout(I.nodes.p, I.n_nodes, (uint32_t)mi, E.tiles.p, E.refs.p + I.first_ref, E.hdr.p, stream)) != hipSuccess) return e;
    }
    E.hdr_host.assign(n_hdr, 0u);
    e = staged_read(stage, E.hdr_host.data(), E.hdr.p, n_hdr * 4, stream);
    E.us[0] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return e;
}

// the gap behind the rec_units units of records and the treelet region zeroed, every mesh's records, the treelets (tl_offset != 0); hdr_host on return
static hipError_t mesh_emit_write(MeshEmit &E, uint8_t *arena, uint32_t rec_units, size_t total_bytes, uint32_t tl_offset, int32_t n_materials, bool timed, PinnedBuf &stage, hipStream_t stream)
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

// ---- the arena of an upload: the host's emit, the device's, and what both refuse ----------------------------------------------------

int mesh_refusal(MeshRefusal why, int mesh, std::string &msg)
{
    static const struct { int code; const char *text; } refusals[] = {{YCGE_ERR_UNSUPPORTED, "mesh %d: a leaf of more than 15 triangles"},
                                                                      {YCGE_ERR_INVALID_ARG, "mesh %d: triangle material out of range"},
                                                                      {YCGE_ERR_UNSUPPORTED, "mesh records exceed the 1 GB arena"}};
    char buf[96];
    std::snprintf(buf, sizeof buf, refusals[why].text, mesh);
    msg = buf;
    return refusals[why].code;
}

// A mesh's device records appended to the arena (32-byte units): depth-first - an internal node (GNode, both child boxes),
// then its left child's records (a leaf's triangle pair records or the whole left subtree), then the right child's - so a
// walk's next fetch is usually the next cache line.  Returns the root reference (ycge_device.h).
static uint32_t emit_mesh_records(const BuiltTree &t, const float *tris9, const int32_t *tri_material, int32_t material, int n_materials,
                                  std::vector<uint8_t> &arena, bool &bad_leaf, bool &bad_material)
{
    if (t.root < 0) return YCGE_REF_NONE_VALUE;
    std::function<uint32_t(int32_t)> emit = [&](int32_t ni) -> uint32_t {
        const RefNode &nd = t.nodes[(size_t)ni];
        const uint32_t unit = (uint32_t)(arena.size() / 32);
        if (nd.count > 0) {
            if (nd.count > 15) { bad_leaf = true; return YCGE_REF_NONE_VALUE; }
            const uint32_t n_rec = ((uint32_t)nd.count + 1u) / 2u;
            arena.resize(arena.size() + (size_t)n_rec * sizeof(GTriPair), 0);        // an odd leaf's last slot stays all zeros
            for (int32_t k = 0; k < nd.count; k++) {
                const int32_t ti = t.leaf_index[(size_t)(nd.start + k)];
                const float *v = tris9 + 9 * (size_t)ti;
                uint8_t *rec = arena.data() + (size_t)unit * 32 + (size_t)(k / 2) * sizeof(GTriPair);
                GTriPair g;
                std::memcpy(&g, rec, sizeof g);
                const int sl = k & 1;
                g.ax[sl] = v[0]; g.ay[sl] = v[1]; g.az[sl] = v[2];
                g.e1x[sl] = v[3] - v[0]; g.e1y[sl] = v[4] - v[1]; g.e1z[sl] = v[5] - v[2];        // MeshBVH.cs:87-91
                g.e2x[sl] = v[6] - v[0]; g.e2y[sl] = v[7] - v[1]; g.e2z[sl] = v[8] - v[2];
                g.orig[sl] = ti;
                g.material[sl] = tri_material ? tri_material[ti] : material;
                if (g.material[sl] < 0 || g.material[sl] >= n_materials) bad_material = true;
                std::memcpy(rec, &g, sizeof g);
            }
            return YCGE_REF(REF_MESH_LEAF, (unit << 4) | (uint32_t)nd.count);
        }
        arena.resize(arena.size() + sizeof(GNode), 0);
        GNode g;
        std::memset(&g, 0, sizeof g);
        const RefNode &L = t.nodes[(size_t)nd.left];
        const RefNode &R = t.nodes[(size_t)nd.right];
        g.lmin_x = L.mn[0]; g.lmin_y = L.mn[1]; g.lmin_z = L.mn[2]; g.lmax_x = L.mx[0]; g.lmax_y = L.mx[1]; g.lmax_z = L.mx[2];
        g.rmin_x = R.mn[0]; g.rmin_y = R.mn[1]; g.rmin_z = R.mn[2]; g.rmax_x = R.mx[0]; g.rmax_y = R.mx[1]; g.rmax_z = R.mx[2];
        g.lref = emit(nd.left);
        g.rref = emit(nd.right);
        std::memcpy(arena.data() + (size_t)unit * 32, &g, sizeof g);
        return YCGE_REF(REF_MESH_NODE, unit << 4);
    };
    return emit(t.root);
}


// Treelets of every internal mesh node (GTreeSlot, ycge_device.h), appended to the arena: a pure function of the records above.
// Returns the region's byte offset, 0 when there is nothing to build or 32-bit offsets would not reach its end.
static uint32_t append_treelets(std::vector<uint8_t> &arena, const std::vector<GMesh> &gmeshes)
{
    bool any = false;
    for (const GMesh &m : gmeshes) any |= YCGE_REF_KIND(m.root_ref) == REF_MESH_NODE && m.root_ref != YCGE_REF_NONE_VALUE;
    size_t total = 0;
    const size_t t0 = mesh_arena_treelet_offset(arena.size(), any, total);          // (shared with the arena assembled on the device: the same answer)
    if (t0 == 0) return 0;
    arena.resize(total, 0);
    auto node_at = [&](uint32_t ref) { GNode g; std::memcpy(&g, arena.data() + (size_t)((ref & 0x1ffffff0u) >> 4) * 32, sizeof g); return g; };
    std::vector<uint32_t> todo;
    for (const GMesh &m : gmeshes) if (m.root_ref != YCGE_REF_NONE_VALUE && YCGE_REF_KIND(m.root_ref) == REF_MESH_NODE) todo.push_back(m.root_ref);
    while (!todo.empty()) {
        const uint32_t ref = todo.back(); todo.pop_back();
        const uint32_t unit = (ref & 0x1ffffff0u) >> 4;
        GTreeSlot slots[YCGE_TL_SLOTS];
        std::memset(slots, 0, sizeof slots);
        // fill(b, parent record): slots 2b+2 / 2b+3 from the record of the node in slot b (b = -1: the treelet's own node)
        std::function<void(int, const GNode &, int)> fill = [&](int b, const GNode &g, int depth) {
            const int l = 2 * b + 2, r = l + 1;
            slots[l].mn[0] = g.lmin_x; slots[l].mn[1] = g.lmin_y; slots[l].mn[2] = g.lmin_z; slots[l].mx_x = g.lmax_x; slots[l].mx_y = g.lmax_y; slots[l].mx_z = g.lmax_z;
            slots[r].mn[0] = g.rmin_x; slots[r].mn[1] = g.rmin_y; slots[r].mn[2] = g.rmin_z; slots[r].mx_x = g.rmax_x; slots[r].mx_y = g.rmax_y; slots[r].mx_z = g.rmax_z;
            slots[l].ref = g.lref; slots[r].ref = g.rref; slots[l].valid = slots[r].valid = 1;
            if (depth < 3)
                for (int c : {l, r})
                    if (YCGE_REF_KIND(slots[c].ref) == REF_MESH_NODE) fill(c, node_at(slots[c].ref), depth + 1);
        };
        const GNode g = node_at(ref);
        fill(-1, g, 1);
        std::memcpy(arena.data() + t0 + (size_t)unit * YCGE_TL_BYTES_PER_UNIT, slots, sizeof slots);
        if (YCGE_REF_KIND(g.lref) == REF_MESH_NODE) todo.push_back(g.lref);
        if (YCGE_REF_KIND(g.rref) == REF_MESH_NODE) todo.push_back(g.rref);
    }
    return (uint32_t)t0;
}

// The host writes the arena: every mesh's records in mesh order, then the treelets
int emit_arena_on_host(const std::vector<MeshHost> &trees, const ycge_mesh *meshes, int n_materials, bool no_coop, std::vector<uint8_t> &arena, std::vector<GMesh> &gmeshes,
                       uint32_t &tl_offset, std::string &msg)
{
    for (size_t mi = 0; mi < trees.size(); mi++) {
        const ycge_mesh &m = meshes[mi];
        bool bad_material = false, bad_leaf = false;
        gmeshes[mi].root_ref = emit_mesh_records(trees[mi].tree, m.triangles, m.tri_material, m.material, n_materials, arena, bad_leaf, bad_material);
        if (bad_leaf) return mesh_refusal(MESH_LEAF_ABOVE_15, (int)mi, msg);
        if (bad_material) return mesh_refusal(MESH_TRI_MATERIAL, (int)mi, msg);
        if (arena.size() / 32 >= (1u << 25)) return mesh_refusal(MESH_ARENA_FULL, (int)mi, msg);
    }
    tl_offset = no_coop ? 0u : append_treelets(arena, gmeshes);
    return YCGE_OK;
}

// The arena of the meshes E holds, assembled on the device: layout, the refusals of the host's emit, the allocation at its exact size,
// records, treelets
int emit_arena_on_device(MeshEmit &E, PinnedBuf &stage, DevBuf<uint8_t> &d_arena, int n_materials, bool no_coop, bool timed, hipStream_t stream, std::vector<uint32_t> &root_refs,
                         uint32_t &tl_offset, std::string &msg)
{
    char buf[256];
    auto hip_bad = [&](const char *what, hipError_t e) {
        (void)hipGetLastError();
        std::snprintf(buf, sizeof buf, "%s failed: %s", what, hipGetErrorString(e)); msg = buf;
        return e == hipErrorOutOfMemory ? YCGE_ERR_OUT_OF_MEMORY : YCGE_ERR_DEVICE;
    };
    hipError_t e = mesh_emit_layout(E, stage, stream);
    if (e != hipSuccess) return hip_bad("the mesh record layout", e);
    const size_t n = E.in.size();
    root_refs.assign(n, YCGE_REF_NONE_VALUE);
    uint64_t units = 0;
    bool any_node_root = false;
    for (size_t mi = 0; mi < n; mi++) {
        const MeshEmit::Input &I = E.in[mi];
        const uint32_t *h = E.hdr_host.data() + 4 + 4 * mi;          // {units, a leaf above 15 triangles, a material out of range, 0}
        if (h[1]) return mesh_refusal(MESH_LEAF_ABOVE_15, (int)mi, msg);
        if (I.n_nodes != 0) {
            if (units < (1u << 25)) root_refs[mi] = I.root_count > 0 ? YCGE_REF(REF_MESH_LEAF, ((uint32_t)units << 4) | (uint32_t)I.root_count) : YCGE_REF(REF_MESH_NODE, (uint32_t)units << 4);
            any_node_root |= I.root_count == 0;
        }
        units += h[0];
        if (units >= (1u << 25)) return mesh_refusal(MESH_ARENA_FULL, (int)mi, msg);
    }
    if (units != E.hdr_host[0]) { msg = "the mesh record layout disagrees with its own total"; return YCGE_ERR_INTERNAL; }
    size_t total = 0;
    tl_offset = no_coop ? 0u : mesh_arena_treelet_offset((size_t)units * 32, any_node_root, total);
    if (tl_offset == 0) total = (size_t)units * 32;
    if ((e = d_arena.alloc(total)) != hipSuccess) return hip_bad("the mesh arena's allocation", e);
    if (total == 0) return YCGE_OK;
    if ((e = mesh_emit_write(E, d_arena.p, (uint32_t)units, total, tl_offset, n_materials, timed, stage, stream)) != hipSuccess) return hip_bad("the mesh records on the device", e);
    for (size_t mi = 0; mi < n; mi++)
        if (E.hdr_host[4 + 4 * mi + 2]) return mesh_refusal(MESH_TRI_MATERIAL, (int)mi, msg);
    return YCGE_OK;
}

uint32_t mesh_tree_units(const BuiltTree &t, bool &bad_leaf)
{
    uint64_t units = 0;
    bad_leaf = false;
    if (t.root < 0) return 0;
    for (const RefNode &nd : t.nodes) {
        if (nd.count > 15) bad_leaf = true;
        else units += nd.count > 0 ? 3u * (((uint32_t)nd.count + 1u) / 2u) : 2u;
    }
    return units > 0xffffffffull ? 0xffffffffu : (uint32_t)units;
}

// The meshes E holds written into an arena that exists (ycge_scene_attach_meshes): the same kernels as emit_arena_on_device, each mesh behind
// its own base unit, the records bounded by the arena's capacity, the treelets of these meshes' nodes alone
int emit_meshes_into_arena(MeshEmit &E, PinnedBuf &stage, uint8_t *arena, uint32_t capacity_units, uint32_t tl_offset, const std::vector<uint32_t> &base_units, const std::vector<uint32_t> &units,
                           int n_materials, hipStream_t stream, std::vector<uint32_t> &root_refs, std::string &msg)
{
    char buf[256];
    auto hip_bad = [&](const char *what, hipError_t e) {
        (void)hipGetLastError();
        std::snprintf(buf, sizeof buf, "%s failed: %s", what, hipGetErrorString(e)); msg = buf;
        return e == hipErrorOutOfMemory ? YCGE_ERR_OUT_OF_MEMORY : YCGE_ERR_DEVICE;
    };
    const size_t n = E.in.size();
    root_refs.assign(n, YCGE_REF_NONE_VALUE);
    hipError_t e = mesh_emit_layout(E, stage, stream, base_units.data());
    if (e != hipSuccess) return hip_bad("the mesh record layout", e);
    for (size_t mi = 0; mi < n; mi++) {
        const MeshEmit::Input &I = E.in[mi];
        const uint32_t *h = E.hdr_host.data() + EH_MESH0 + EH_MESH_WORDS * mi;
        if (h[1]) return mesh_refusal(MESH_LEAF_ABOVE_15, (int)mi, msg);
        if (I.n_nodes == 0) continue;
        if (h[0] != units[mi] || (uint64_t)base_units[mi] + units[mi] > capacity_units) { msg = "the mesh record layout disagrees with the host's count"; return YCGE_ERR_INTERNAL; }
        root_refs[mi] = I.root_count > 0 ? YCGE_REF(REF_MESH_LEAF, (base_units[mi] << 4) | (uint32_t)I.root_count) : YCGE_REF(REF_MESH_NODE, base_units[mi] << 4);
    }
    if ((e = mesh_emit_write(E, arena, capacity_units, 0, tl_offset, n_materials, false, stage, stream)) != hipSuccess) return hip_bad("the mesh records on the device", e);
    for (size_t mi = 0; mi < n; mi++)
        if (E.hdr_host[EH_MESH0 + EH_MESH_WORDS * mi + 2]) return mesh_refusal(MESH_TRI_MATERIAL, (int)mi, msg);
    return YCGE_OK;
}

// a hook's read of what c's device holds at src, into dst (null: nothing to read) once the device is idle
static int read_idle_device(ycge_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (!dst || bytes == 0) return YCGE_OK;
    HIP_TRY(c, hipDeviceSynchronize());
    return copy_out(c, dst, src, bytes);
}

// one mesh (single material 0) through the host builder and the host's emit, treelets on request; the arena's size, its bytes when they fit
static int host_arena_of_one_mesh(const float *tris9, int32_t n, bool treelets, void *out, int64_t capacity_bytes, uint32_t *root_ref_out, uint32_t *tl_offset_out)
{
    std::vector<MeshHost> trees(1);
    host_mesh_tree(tris9, n, trees[0].tree);
    ycge_mesh m;
    std::memset(&m, 0, sizeof m);
    m.triangles = tris9; m.n_triangles = n;
    std::vector<uint8_t> arena;
    std::vector<GMesh> gmeshes(1, GMesh{});
    std::string msg;
    uint32_t tl_offset = 0;
    const int rc = emit_arena_on_host(trees, &m, 1, !treelets, arena, gmeshes, tl_offset, msg);
    *root_ref_out = gmeshes[0].root_ref;
    if (rc != YCGE_OK) return YCGE_ERR_UNSUPPORTED;
    if (tl_offset_out) *tl_offset_out = tl_offset;
    if (out && (int64_t)arena.size() <= capacity_bytes && !arena.empty()) std::memcpy(out, arena.data(), arena.size());
    return (int)arena.size();
}

} // namespace ycge_host

// ---- the hooks of the mesh path (tests and profiles hold the builders and the two emits by them) ------------------------------------------
extern "C" {

// test hook, no context: the builder alone on the current device, with ycge_scene_upload's answer to what it declines (the host builds
// the mesh).  nodes_out: 2 n records of 40 bytes, leaf_out: n.  res16: {depth, Array.Sort cases, wide nodes, subtree workgroups, fallback
// reason (MESH_BVH_*, 0 = built on the device), 1 = built on the device, wide levels, microseconds of the device build}.  Returns the node
// count; YCGE_ERR_NO_DEVICE_CODE without a device, nothing written.  YCGE_MESH_BVH_WIDE_MIN is read at every call.
int ycge_debug_device_mesh_bvh(const float *tris9, int32_t n, void *nodes_out, int32_t *leaf_out, uint32_t *res16)
try {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { (void)hipGetLastError(); return YCGE_ERR_NO_DEVICE_CODE; }
    if (n < 0 || !res16 || (n > 0 && (!tris9 || !nodes_out || !leaf_out))) return YCGE_ERR_INVALID_ARG;
    Knobs knobs;
    knobs.read();
    MeshBvhScratch scratch;
    MeshBvhReport rep;
    BuiltTree t;
    bool on_device = false;
    const int rc = build_mesh_tree(knobs, true, scratch, tris9, n, nullptr, t, on_device, rep);
    if (rc < 0) return rc;
    for (int k = 0; k < 16; k++) res16[k] = 0u;
    res16[0] = (uint32_t)t.max_depth; res16[1] = (uint32_t)t.sort_fallbacks; res16[2] = (uint32_t)rep.wide_nodes; res16[3] = (uint32_t)rep.jobs;
    res16[4] = (uint32_t)rep.fallback; res16[5] = on_device ? 1u : 0u; res16[6] = (uint32_t)rep.levels; res16[7] = (uint32_t)rep.us;
    return tree_out(t, nodes_out, leaf_out, nullptr);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test / profiling hook: how ycge_scene_upload built the mesh BVHs - {device builds, host builds, host builds after the device builder
// declined (counted in host builds too), microseconds of the last device build (items kernel to the tree in host memory), and of the last
// upload: Array.Sort cases, deepest tree, wide nodes, subtree workgroups}.  Without a context: YCGE_ERR_INVALID_ARG, and out8[0..2] = the
// three knobs as the environment gives them now (YCGE_MESH_BVH_HOST, _DEVICE_MIN, _WIDE_MIN after its clamp) - host only, no device.
int ycge_debug_mesh_bvh_stats(ycge_ctx *c, int64_t *out8)
try {
    if (!out8) return YCGE_ERR_INVALID_ARG;
    if (!c) {
        Knobs knobs;
        knobs.read();
        for (int k = 0; k < 8; k++) out8[k] = 0;
        out8[0] = knobs.mesh_bvh_host ? 1 : 0; out8[1] = knobs.mesh_bvh_device_min; out8[2] = knobs.mesh_bvh_wide_min;
        return YCGE_ERR_INVALID_ARG;
    }
    out8[0] = c->mesh_bvh_device_builds; out8[1] = c->mesh_bvh_host_builds; out8[2] = c->mesh_bvh_host_fallbacks; out8[3] = (int64_t)c->mesh_bvh_last_us;
    out8[4] = c->mesh_bvh_sorts; out8[5] = c->mesh_bvh_depth; out8[6] = c->mesh_bvh_wide_nodes; out8[7] = c->mesh_bvh_jobs;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook, no context: the twin of ycge_host_mesh_arena_treelets on the current device - the tree (the device builder, or the
// host's tree uploaded when that declines), then the kernels of ycge_mesh_emit.hip; single material 0.  Returns the arena's size, the bytes
// in `out` when they fit.  res8: {1 = tree built on the device, nodes, units of records, us of the layout, of the records, of the treelets
// (each with its wait), 0, 0}.  YCGE_ERR_NO_DEVICE_CODE without a device, nothing written.  YCGE_MESH_BVH_WIDE_MIN and YCGE_NO_COOP are read at every call.
int ycge_debug_device_mesh_arena(const float *tris9, int32_t n, void *out, int64_t capacity_bytes, uint32_t *root_ref_out, uint32_t *tl_offset_out, uint32_t *res8)
try {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { (void)hipGetLastError(); return YCGE_ERR_NO_DEVICE_CODE; }
    if (n < 0 || (n > 0 && !tris9) || !root_ref_out || !tl_offset_out) return YCGE_ERR_INVALID_ARG;
    Knobs knobs;
    knobs.read();
    MeshBvhScratch scratch;
    MeshEmit E;
    MeshBvhReport rep;
    BuiltTree t;
    bool on_device = false;
    const int rc = build_mesh_tree(knobs, true, scratch, tris9, n, nullptr, t, on_device, rep);
    if (rc < 0) return rc;
    on_device = on_device && n > 0;
    if (mesh_emit_add(E, 0, on_device, scratch, t, tris9, n, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); return YCGE_ERR_DEVICE; }
    DevBuf<uint8_t> d_arena;
    std::vector<uint32_t> root_refs;
    std::string msg;
    *tl_offset_out = 0;
    const int erc = emit_arena_on_device(E, scratch.stage, d_arena, 1, knobs.no_coop, true, nullptr, root_refs, *tl_offset_out, msg);
    if (erc != YCGE_OK) return erc == YCGE_ERR_INVALID_ARG ? YCGE_ERR_UNSUPPORTED : erc;          // (as the host twin answers a bad leaf or material)
    *root_ref_out = root_refs[0];
    if (d_arena.n > (size_t)0x7fffffff) return YCGE_ERR_UNSUPPORTED;
    if (out && (int64_t)d_arena.n <= capacity_bytes && d_arena.n) {          // (through page-locked staging: the device writes no caller memory)
        const hipError_t e = staged_read(scratch.stage, out, d_arena.p, d_arena.n, nullptr);
        if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? YCGE_ERR_OUT_OF_MEMORY : YCGE_ERR_DEVICE; }
    }
    if (res8) {
        for (int k = 0; k < 8; k++) res8[k] = 0u;
        res8[0] = on_device ? 1u : 0u; res8[1] = (uint32_t)t.nodes.size(); res8[2] = E.hdr_host.empty() ? 0u : E.hdr_host[0];
        res8[3] = (uint32_t)E.us[0]; res8[4] = (uint32_t)E.us[1]; res8[5] = (uint32_t)E.us[2];
    }
    return (int)d_arena.n;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: the arena the context's device holds (records, then the treelet region at *tl_offset_out, 0 = none), whichever side wrote it.
// Returns its size; the bytes go to dst when they fit.
int ycge_debug_read_mesh_arena(ycge_ctx *c, void *dst, int64_t capacity_bytes, uint32_t *tl_offset_out)
try {
    if (!c || !tl_offset_out) return YCGE_ERR_INVALID_ARG;
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    *tl_offset_out = c->sd.tl_offset;
    const size_t bytes = c->d_mesh_arena.p ? c->d_mesh_arena.n : 0;
    if (bytes > (size_t)0x7fffffff) return c->fail(YCGE_ERR_UNSUPPORTED, "the arena is larger than this hook returns");
    const int rc = read_idle_device(c, (int64_t)bytes <= capacity_bytes ? dst : nullptr, c->d_mesh_arena.p, bytes);
    return rc != YCGE_OK ? rc : (int)bytes;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the GMesh records (32 bytes each: root box, root reference) the context's device holds; returns how many
int ycge_debug_read_meshes(ycge_ctx *c, void *dst, int32_t capacity_meshes)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    const size_t n = c->d_meshes.p ? c->d_meshes.n : 0;
    const int rc = read_idle_device(c, n <= (size_t)(capacity_meshes > 0 ? capacity_meshes : 0) ? dst : nullptr, c->d_meshes.p, n * sizeof(GMesh));
    return rc != YCGE_OK ? rc : (int)n;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: who wrote the arena of the last upload - {meshes whose records the device wrote, meshes whose records the host
// wrote, microseconds of the device's layout + records + treelets (0: the host wrote them), the arena's bytes}.  Without a context:
// YCGE_ERR_INVALID_ARG, and out4[0..1] = YCGE_MESH_EMIT_HOST and YCGE_MESH_EMIT_DEVICE_MIN as the environment gives them now (host only).
int ycge_debug_mesh_emit_stats(ycge_ctx *c, int64_t *out4)
try {
    if (!out4) return YCGE_ERR_INVALID_ARG;
    if (!c) {
        Knobs knobs;
        knobs.read();
        out4[0] = knobs.mesh_emit_host ? 1 : 0; out4[1] = knobs.mesh_emit_device_min; out4[2] = out4[3] = 0;
        return YCGE_ERR_INVALID_ARG;
    }
    out4[0] = c->mesh_emit_dev_meshes; out4[1] = c->mesh_emit_host_meshes; out4[2] = (int64_t)c->mesh_emit_last_us; out4[3] = c->mesh_emit_arena_bytes;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: the resident meshes of the context's scene - {resident meshes, free indices, units of records in use, capacity in units
// (before the first attach: the uploaded records), growths of the pooled arena, ranges reused, device builds, host builds of the attaches, then the
// last attach in microseconds: the trees, the emit, the copies (re-homing, growth, other devices), and 1 once the arena is pooled}
int ycge_debug_mesh_pool_stats(ycge_ctx *c, int64_t *out12)
try {
    if (!c || !out12) return YCGE_ERR_INVALID_ARG;
    return mesh_pool_stats(c, out12);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook, no context and no device: the pool's allocator of unit ranges and mesh indices (MeshRanges, ycge_mesh_pool.h) run through n_ops
// triples {op, a, b} from `end0` units of records and `n_index0` indices - 0: take a units, 1: give back the b units at unit a, 2: take an
// index, 3: give back index a.  out: per op {the take's answer, the records' end, free ranges, free units}
int ycge_debug_mesh_ranges(int64_t end0, int32_t n_index0, const int64_t *ops, int32_t n_ops, int64_t *out)
try {
    if (end0 < 0 || n_index0 < 0 || n_ops < 0 || (n_ops > 0 && (!ops || !out))) return YCGE_ERR_INVALID_ARG;
    mesh_ranges_run(end0, n_index0, ops, n_ops, out);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ---- host-only helpers exported for the `-m "not gpu"` tests (no device needed) -------------
// Build a tree over caller-supplied boxes with the product builder: bounds = n*6 (min xyz, max xyz),
// centroids = n*3.  flavour 0 = scene, 1 = mesh.  Outputs are malloc'ed by the caller:
// nodes_out must hold 2*n records of 10 x 4 B, leaf_out n int32.  Returns node count or <0.
int ycge_host_build_tree(const float *bounds, const float *centroids, int32_t n, int32_t flavour, void *nodes_out, int32_t *leaf_out,
                         int32_t *stats_out /* [root, max_depth, sort_fallbacks] */)
try {
    if (n < 0 || (n > 0 && (!bounds || !centroids || !nodes_out || !leaf_out))) return YCGE_ERR_INVALID_ARG;
    BoundsSoA it;
    it.resize(n);
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) { it.mn[a][i] = bounds[6 * i + a]; it.mx[a][i] = bounds[6 * i + 3 + a]; it.c[a][i] = centroids[3 * i + a]; }
    BuiltTree t;
    build_tree(it, flavour == 0 ? TreeFlavour::Scene : TreeFlavour::Mesh, t);
    return tree_out(t, nodes_out, leaf_out, stats_out);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// Same for a triangle soup (MeshBVH ctor path incl. TryComputeBounds).
int ycge_host_build_mesh(const float *tris9, int32_t n, void *nodes_out, int32_t *leaf_out, int32_t *stats_out)
try {
    if (n < 0 || (n > 0 && (!tris9 || !nodes_out || !leaf_out))) return YCGE_ERR_INVALID_ARG;
    BuiltTree t;
    host_mesh_tree(tris9, n, t);
    return tree_out(t, nodes_out, leaf_out, stats_out);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: the device records of one mesh (single material 0) as emit_mesh_records lays them out
int ycge_host_mesh_arena(const float *tris9, int32_t n, void *out, int64_t capacity_bytes, uint32_t *root_ref_out)
try {
    if (n < 0 || (n > 0 && !tris9) || !root_ref_out) return YCGE_ERR_INVALID_ARG;
    return host_arena_of_one_mesh(tris9, n, false, out, capacity_bytes, root_ref_out, nullptr);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ... with the treelet region of the cooperative walk appended (append_treelets): returns the total size, *tl_offset_out = where it starts
int ycge_host_mesh_arena_treelets(const float *tris9, int32_t n, void *out, int64_t capacity_bytes, uint32_t *root_ref_out, uint32_t *tl_offset_out)
try {
    if (n < 0 || (n > 0 && !tris9) || !root_ref_out || !tl_offset_out) return YCGE_ERR_INVALID_ARG;
    return host_arena_of_one_mesh(tris9, n, true, out, capacity_bytes, root_ref_out, tl_offset_out);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

} // extern "C"

