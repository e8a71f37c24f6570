// ycge_mesh_pool.cpp - meshes and materials of a resident scene: the bodies of ycge_scene_attach_meshes / _detach_meshes /
// _append_materials / _attach_obj_mesh (exported from ycge_scene.cpp) and the pool of resident meshes behind them.
//
// A mesh record is addressed by an absolute 32-byte unit from SceneDev::mesh_arena, and the treelet of the node at unit u lies at
// tl_offset + u * YCGE_TL_BYTES_PER_UNIT: both maps are linear, so a mesh can be written at ANY base unit of an arena with room, and no
// frame or query kernel needs to know.  ycge_scene_upload still lays the arena out at its exact size (MeshPool::pooled == false); the first
// attach re-homes it into [records: capacity units][treelets at the 512-aligned tl_offset] - records keep their units, the treelet region is
// copied to the new tl_offset - and growth (geometric) is the same two device copies.  Free ranges: MeshRanges (ycge_mesh_pool.h).
//
// ONE WRITE PATH: every attached mesh - its tree built on the device or by the host (build_mesh_tree, the knobs and fallbacks of an upload)
// - goes through the kernels of ycge_mesh_emit.hip (emit_meshes_into_arena, ycge_mesh_bvh.cpp), each behind its own base unit.  The range a
// mesh takes is zeroed first, records and treelet slots: k_emit_treelets and an odd leaf's empty slot rely on zeros.
//
// ALL OR NOTHING: every refusal - arguments, a leaf above 15 triangles, a tree deeper than 64, the pool's limit - is decided before the
// pool is touched; the plan is made on a copy of the pool, which replaces it in a last step that cannot fail.  A re-homed or grown arena
// stays when a later device call fails: its contents are what they were, nothing refers to the new room.
//
// SEVERAL DEVICES: the root builds and emits once; every other device receives the new record ranges and treelet ranges by a device copy.
//
// FRAMES IN FLIGHT: an attach and an append join them (quiesce_all): the arena and the tables may move.  A detach changes host state only.
// What SceneDev tells the kernels about the resident set - tl_offset (0 while no resident mesh has a node root, as an upload of the
// equivalent scene leaves it), the flags of the material list - follows the set with the next install of the objects (mesh_pool_publish).
#include <algorithm>

#include "ycge_ctx.h"

namespace ycge_host {

namespace {

bool root_is_a_node(const GMesh &g) { return g.root_ref != YCGE_REF_NONE_VALUE && YCGE_REF_KIND(g.root_ref) == REF_MESH_NODE; }

bool any_node_root(const ycge_ctx *c)
{
    const MeshPool &P = c->mesh_pool;
    for (size_t i = 0; i < c->gmeshes_host.size() && i < P.resident.size(); i++)
        if (P.resident[i] && root_is_a_node(c->gmeshes_host[i])) return true;
    return false;
}

// the most units of records a pooled arena may have room for: every unit addressable by a reference's 25 bits and, with treelets, the
// region's end within 32-bit offsets (mesh_arena_treelet_offset's condition); YCGE_MESH_POOL_MAX_UNITS lowers it
uint64_t pool_limit_units(const ycge_ctx *c, bool treelets)
{
    uint64_t limit = (uint64_t)1 << 25;
    if (treelets) limit = std::min<uint64_t>(limit, (((uint64_t)1 << 32) - 4096 - 512 - 1) / (32 + YCGE_TL_BYTES_PER_UNIT));
    if (c->knobs.mesh_pool_max_units > 0) limit = std::min<uint64_t>(limit, (uint64_t)c->knobs.mesh_pool_max_units);
    return limit;
}

// SceneDev::tl_offset as an upload of the equivalent scene leaves it, on every device
void publish_arena(ycge_ctx *c)
{
    const MeshPool &P = c->mesh_pool;
    const uint32_t tl = P.tl_offset != 0 && any_node_root(c) ? P.tl_offset : 0u;
    auto publish = [&](ycge_ctx *x) { x->sd.mesh_arena = x->d_mesh_arena.p; x->sd.tl_offset = tl; };          // (no allocation: this runs inside steps that cannot fail)
    publish(c);
    for (ycge_ctx *p : c->peers) publish(p);
}

// the deepest resident tree, where check_scene_depth reads it (host state alone: the next install of the objects sizes the spill columns by it)
void publish_depth(ycge_ctx *c)
{
    const MeshPool &P = c->mesh_pool;
    int depth = 0;
    for (size_t i = 0; i < c->meshes.size() && i < P.resident.size(); i++)
        if (P.resident[i] && c->meshes[i].tree.max_depth > depth) depth = c->meshes[i].tree.max_depth;
    c->max_mesh_depth = depth;
    for (ycge_ctx *p : c->peers) p->max_mesh_depth = depth;
}

// The arena of every device re-homed into an allocation of `capacity` units: zeros, then the records at their units and the treelet region
// at the new tl_offset.  Every larger arena is made and filled before any device takes its own.
int rehome(ycge_ctx *c, MeshPool &P, uint64_t capacity)
{
    MeshPool &L = c->mesh_pool;
    const uint64_t old_end = L.ranges.end;
    const size_t rec_bytes = (size_t)capacity * 32;
    const uint32_t new_tl = L.treelets ? (uint32_t)((rec_bytes + 511) & ~(size_t)511) : 0u;
    const size_t total = L.treelets ? (size_t)new_tl + (size_t)capacity * YCGE_TL_BYTES_PER_UNIT : rec_bytes;
    const std::vector<ycge_ctx *> ctxs = contexts_of(c);
    std::vector<DevBuf<uint8_t>> larger(ctxs.size());
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < ctxs.size() && e == hipSuccess; i++) {
        ycge_ctx *x = ctxs[i];
        e = hipSetDevice(x->device);
        if (e == hipSuccess) e = larger[i].alloc(total);
        if (e == hipSuccess) e = hipMemset(larger[i].p, 0, total);
        if (e == hipSuccess && old_end && x->d_mesh_arena.p) e = hipMemcpy(larger[i].p, x->d_mesh_arena.p, (size_t)old_end * 32, hipMemcpyDeviceToDevice);
        if (e == hipSuccess && old_end && x->d_mesh_arena.p && new_tl && L.tl_offset)
            e = hipMemcpy(larger[i].p + new_tl, x->d_mesh_arena.p + L.tl_offset, (size_t)old_end * YCGE_TL_BYTES_PER_UNIT, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    (void)hipSetDevice(c->device);
    HIP_TRY(c, e);
    for (size_t i = 0; i < ctxs.size(); i++) ctxs[i]->d_mesh_arena = std::move(larger[i]);
    if (L.pooled) { L.growths++; P.growths++; }
    L.pooled = P.pooled = true;
    L.capacity = P.capacity = capacity;
    L.tl_offset = P.tl_offset = new_tl;
    publish_arena(c);
    return YCGE_OK;
}

} // namespace

void mesh_pool_reset(ycge_ctx *c, uint32_t tl_offset)
{
    MeshPool P;
    const size_t n = c->meshes.size();
    P.resident.assign(n, 1); P.first_unit.assign(n, 0); P.units.assign(n, 0);
    bool any_node = false;
    for (size_t i = 0; i < n; i++) {
        bool bad_leaf = false;
        P.units[i] = mesh_tree_units(c->meshes[i].tree, bad_leaf);
        P.first_unit[i] = P.ranges.end;
        P.ranges.end += P.units[i];
        if (i < c->gmeshes_host.size()) any_node |= root_is_a_node(c->gmeshes_host[i]);
    }
    P.ranges.n_index = (int32_t)n;
    P.n_resident = (int64_t)n;
    P.units_in_use = (int64_t)P.ranges.end;
    P.tl_offset = tl_offset;
    P.treelets = !c->knobs.no_coop && !(any_node && tl_offset == 0);          // (an upload too large for a treelet region: the pool has none either)
    c->mesh_pool = std::move(P);
    c->pending_transparent = c->pending_textured = false;
}

void mesh_pool_publish(ycge_ctx *c)
{
    publish_depth(c);
    publish_arena(c);
    auto publish = [&](ycge_ctx *x) {
        if (c->pending_transparent) x->sd.any_transparent = 1;
        if (c->pending_textured) x->sd.any_textured = 1;
    };
    publish(c);
    for (ycge_ctx *p : c->peers) publish(p);
    c->pending_transparent = c->pending_textured = false;
}

// the body of ycge_scene_attach_meshes; d_tris9: meshes[0].triangles is NULL and its soup lies on the root's device (n == 1, ycge_scene_attach_obj_mesh)
static int attach_meshes_from(ycge_ctx *c, const ycge_mesh *meshes, int32_t n, int32_t *out_mesh_index, const float *d_tris9)
{
    auto mat_ok = [&](int mi) { return mi >= 0 && mi < c->n_materials; };
    std::string msg;
    for (int k = 0; k < n; k++) {
        const ycge_mesh &m = meshes[k];
        if (m.n_triangles < 0 || (m.n_triangles > 0 && !m.triangles && !d_tris9)) return c->fail(YCGE_ERR_INVALID_ARG, "mesh %d: bad triangle array", k);
        if (!m.tri_material && !mat_ok(m.material)) return c->fail(YCGE_ERR_INVALID_ARG, "mesh %d: material out of range", k);
        if (m.tri_material)
            for (int t = 0; t < m.n_triangles; t++)
                if (!mat_ok(m.tri_material[t])) { const int rc = mesh_refusal(MESH_TRI_MATERIAL, k, msg); return c->fail(rc, "%s", msg.c_str()); }
    }
    int rc = quiesce_all(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const DeviceGuard guard(c->device);
    const Knobs &knobs = c->knobs;
    MeshEmit &E = c->mesh_emit;
    MeshUploadScratch scratch_of_this_attach{c->mesh_bvh, E};
    E.release();

    // ---- every tree and every verdict
    auto t0 = std::chrono::steady_clock::now();
    std::vector<BuiltTree> trees((size_t)n);
    std::vector<uint32_t> units((size_t)n, 0u);
    std::vector<float> soup;          // a device soup the host builder has to see: read back once
    int64_t device_builds = 0, host_builds = 0;
    for (int k = 0; k < n; k++) {
        const ycge_mesh &m = meshes[k];
        BuiltTree &t = trees[(size_t)k];
        const float *tris = m.triangles;
        bool on_device = false;
        MeshBvhReport rep;
        int brc = build_mesh_tree(knobs, false, c->mesh_bvh, tris, m.n_triangles, c->stream, t, on_device, rep, d_tris9);
        if (brc == 1) {          // below YCGE_MESH_BVH_DEVICE_MIN, or the device builder declined it
            soup.resize((size_t)9 * m.n_triangles);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            rc = copy_out(c, soup.data(), d_tris9, soup.size() * sizeof(float));
            if (rc != YCGE_OK) return rc;
            tris = soup.data();
            Knobs host_only = knobs;
            host_only.mesh_bvh_host = true;
            brc = build_mesh_tree(host_only, false, c->mesh_bvh, tris, m.n_triangles, c->stream, t, on_device, rep);
        }
        if (brc < 0) return c->fail(brc, "mesh %d: device-side BVH build failed: %s", k, hipGetErrorString(rep.error));
        (on_device ? device_builds : host_builds)++;
        if (t.max_depth > 64) return c->fail(YCGE_ERR_STACK_DEPTH, "mesh %d: BVH depth %d exceeds the reference's 64-entry stack (MeshBVH.cs:150)", k, t.max_depth);
        bool bad_leaf = false;
        units[(size_t)k] = mesh_tree_units(t, bad_leaf);
        if (bad_leaf) { rc = mesh_refusal(MESH_LEAF_ABOVE_15, k, msg); return c->fail(rc, "%s", msg.c_str()); }
        HIP_TRY(c, mesh_emit_add(E, (size_t)k, on_device, c->mesh_bvh, t, tris, m.n_triangles, m.tri_material, m.material));
    }
    const double us_build = us_since(t0);

    // ---- the plan, on a copy of the pool: indices (lowest free first), ranges (first fit by address, else the end of the records)
    MeshPool P = c->mesh_pool;
    std::vector<int32_t> index((size_t)n);
    std::vector<uint32_t> base((size_t)n, 0u);
    for (int k = 0; k < n; k++) {
        const int32_t i = P.ranges.take_index();
        const uint64_t first = P.ranges.take(units[(size_t)k]);
        if ((size_t)P.ranges.n_index > P.resident.size()) { P.resident.resize((size_t)P.ranges.n_index, 0); P.first_unit.resize((size_t)P.ranges.n_index, 0); P.units.resize((size_t)P.ranges.n_index, 0); }
        index[(size_t)k] = i;
        base[(size_t)k] = (uint32_t)std::min<uint64_t>(first, 0xffffffffu);
        P.resident[(size_t)i] = 1; P.first_unit[(size_t)i] = first; P.units[(size_t)i] = units[(size_t)k];
        P.n_resident++; P.units_in_use += units[(size_t)k];
    }
    P.device_builds += device_builds; P.host_builds += host_builds;
    const uint64_t limit = pool_limit_units(c, P.treelets);
    if (P.ranges.end > limit)
        return c->fail(YCGE_ERR_UNSUPPORTED, "mesh records exceed the pool's limit of %llu bytes", (unsigned long long)limit * 32ull);

    // ---- room: the first attach re-homes the arena, a later one grows it
    t0 = std::chrono::steady_clock::now();
    if (!P.pooled || P.ranges.end > P.capacity) {
        uint64_t want = P.pooled ? 2 * P.capacity
                                 : knobs.mesh_pool_units > 0 ? (uint64_t)knobs.mesh_pool_units : std::max<uint64_t>(2 * c->mesh_pool.ranges.end, ((uint64_t)1 << 20) / 32);
        want = std::min<uint64_t>(std::max<uint64_t>(want, std::max<uint64_t>(P.ranges.end, 1)), limit);
        rc = rehome(c, P, want);
        if (rc != YCGE_OK) return rc;
    }
    double us_copy = us_since(t0);

    // ---- the records at their base units and the treelets of exactly the new nodes, on the root's device
    t0 = std::chrono::steady_clock::now();
    uint8_t *arena = c->d_mesh_arena.p;
    for (int k = 0; k < n; k++) {
        const size_t u = units[(size_t)k], b = base[(size_t)k];
        if (u == 0) continue;
        HIP_TRY(c, hipMemsetAsync(arena + b * 32, 0, u * 32, c->stream));
        if (P.tl_offset) HIP_TRY(c, hipMemsetAsync(arena + P.tl_offset + b * YCGE_TL_BYTES_PER_UNIT, 0, u * YCGE_TL_BYTES_PER_UNIT, c->stream));
    }
    std::vector<uint32_t> root_refs;
    rc = emit_meshes_into_arena(E, c->mesh_bvh.stage, arena, (uint32_t)P.capacity, P.tl_offset, base, units, c->n_materials, c->stream, root_refs, msg);
    if (rc != YCGE_OK) return c->fail(rc, "%s", msg.c_str());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double us_emit = us_since(t0);

    // ---- the other devices: the new ranges by a device copy
    t0 = std::chrono::steady_clock::now();
    for (ycge_ctx *p : c->peers) {
        HIP_TRY(c, hipSetDevice(p->device));
        for (int k = 0; k < n; k++) {
            const size_t u = units[(size_t)k], b = base[(size_t)k];
            if (u == 0) continue;
            const size_t at[2] = {b * 32, (size_t)P.tl_offset + b * YCGE_TL_BYTES_PER_UNIT}, len[2] = {u * 32, u * YCGE_TL_BYTES_PER_UNIT};
            for (int part = 0; part < (P.tl_offset ? 2 : 1); part++) {
                if (p->device == c->device) HIP_TRY(c, hipMemcpy(p->d_mesh_arena.p + at[part], arena + at[part], len[part], hipMemcpyDeviceToDevice));
                else HIP_TRY(c, hipMemcpyPeer(p->d_mesh_arena.p + at[part], p->device, arena + at[part], c->device, len[part]));
            }
        }
        HIP_TRY(c, hipDeviceSynchronize());
    }
    HIP_TRY(c, hipSetDevice(c->device));

    // ---- the mesh table
    std::vector<GMesh> gmeshes = c->gmeshes_host;
    GMesh none;
    std::memset(&none, 0, sizeof none);
    none.root_ref = YCGE_REF_NONE_VALUE;
    gmeshes.resize((size_t)P.ranges.n_index, none);
    for (int k = 0; k < n; k++) {
        GMesh &gm = gmeshes[(size_t)index[(size_t)k]];
        const BuiltTree &t = trees[(size_t)k];
        gm = none;
        if (t.root >= 0) for (int a = 0; a < 3; a++) { gm.root_min[a] = t.nodes[t.root].mn[a]; gm.root_max[a] = t.nodes[t.root].mx[a]; }
        gm.root_ref = root_refs[(size_t)k];
    }
    for (ycge_ctx *x : contexts_of(c)) {
        HIP_TRY(c, hipSetDevice(x->device));
        HIP_TRY(c, x->d_meshes.upload(gmeshes));
        x->sd.meshes = x->d_meshes.p;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    us_copy += us_since(t0);
    std::vector<MeshHost> hosts((size_t)P.ranges.n_index);          // (made before the step that cannot fail: the only allocation it would need)
    HIP_TRY(c, c->scene_ev.ensure());                               // (... and the event the scene queries wait for)

    // ---- nothing below fails
    for (size_t i = 0; i < hosts.size() && i < c->meshes.size(); i++) hosts[i].tree = std::move(c->meshes[i].tree);
    for (int k = 0; k < n; k++) hosts[(size_t)index[(size_t)k]].tree = std::move(trees[(size_t)k]);
    c->meshes.swap(hosts);
    c->gmeshes_host.swap(gmeshes);
    P.last_attach_us[0] = us_build; P.last_attach_us[1] = us_emit; P.last_attach_us[2] = us_copy;
    c->mesh_pool = std::move(P);
    publish_arena(c);
    publish_depth(c);
    for (int k = 0; k < n; k++) out_mesh_index[k] = index[(size_t)k];
    // the scene queries' mark behind this change: everything above has been waited for, so a record that fails loses nothing
    if (hipEventRecord(c->scene_ev, c->stream) != hipSuccess) (void)hipGetLastError();
    return YCGE_OK;
}

int scene_attach_meshes(ycge_ctx *c, const ycge_mesh *meshes, int32_t n, int32_t *out_mesh_index) { return attach_meshes_from(c, meshes, n, out_mesh_index, nullptr); }

int scene_attach_device_soup(ycge_ctx *c, const float *d_tris9, int32_t n_triangles, int32_t material, int32_t *out_mesh_index)
{
    ycge_mesh m;
    std::memset(&m, 0, sizeof m);
    m.n_triangles = n_triangles; m.material = material;
    return attach_meshes_from(c, &m, 1, out_mesh_index, n_triangles > 0 ? d_tris9 : nullptr);
}

int scene_detach_meshes(ycge_ctx *c, const int32_t *mesh_index, int32_t n)
{
    MeshPool P = c->mesh_pool;
    for (int k = 0; k < n; k++) {
        const int32_t mi = mesh_index[k];
        if (mi < 0 || (size_t)mi >= c->mesh_pool.resident.size() || !c->mesh_pool.resident[(size_t)mi])
            return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_meshes: mesh %d is not resident", mi);
        if (!P.resident[(size_t)mi]) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_meshes: mesh %d is named twice", mi);
        for (size_t i = 0; i < c->last_prims.size(); i++)
            if (c->last_prims[i].type == YCGE_PRIM_MESH && c->last_prims[i].ref == mi)
                return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_meshes: mesh %d is held by object %d of Scene.Objects", mi, (int)i);
        const size_t i = (size_t)mi;
        P.ranges.give(P.first_unit[i], P.units[i]);
        P.ranges.give_index(mi);
        P.n_resident--; P.units_in_use -= P.units[i];
        P.resident[i] = 0; P.first_unit[i] = 0; P.units[i] = 0;
    }
    const size_t n_index = (size_t)P.ranges.n_index;          // the tables follow the resident set: free indices at the end go
    P.resident.resize(n_index); P.first_unit.resize(n_index); P.units.resize(n_index);
    // ---- nothing below fails (the vectors only shrink)
    GMesh none;
    std::memset(&none, 0, sizeof none);
    none.root_ref = YCGE_REF_NONE_VALUE;
    for (int k = 0; k < n; k++) { c->gmeshes_host[(size_t)mesh_index[k]] = none; c->meshes[(size_t)mesh_index[k]] = MeshHost{}; }
    c->gmeshes_host.resize(n_index, none);
    c->meshes.resize(n_index);
    c->mesh_pool = std::move(P);
    publish_depth(c);
    return YCGE_OK;
}

int scene_append_materials(ycge_ctx *c, const ycge_material *materials, int32_t n, int32_t *out_first_index)
{
    const int n_textures = (int)(c->tex_info_host.size() / 4);
    for (int k = 0; k < n; k++) {
        const ycge_material &m = materials[k];
        if (m.kind == YCGE_MAT_TEXTURED) {
            if (m.texture < 0 || m.texture >= n_textures)
                return c->fail(YCGE_ERR_INVALID_ARG, "material %d: texture index %d out of range (%d textures)", c->n_materials + k, m.texture, n_textures);
        } else if (m.kind != YCGE_MAT_CONSTANT && m.kind != YCGE_MAT_CHECKER) return c->fail(YCGE_ERR_UNSUPPORTED, "material %d: unknown kind %d", c->n_materials + k, m.kind);
    }
    if ((long long)c->n_materials + n > 0x7fffffffll) return c->fail(YCGE_ERR_UNSUPPORTED, "more than 2^31 materials");
    int rc = quiesce_all(c);
    if (rc != YCGE_OK) return rc;
    const DeviceGuard guard(c->device);
    std::vector<GMaterial> mats((size_t)n);
    bool transparent = false, textured = false, can_mirror = false;
    for (int k = 0; k < n; k++) {
        flatten_material(materials[k], mats[(size_t)k], transparent, textured);
        if (materials[k].reflectivity >= c->cfg.mirror_threshold) can_mirror = true;
    }
    const size_t have = (size_t)c->n_materials;
    const std::vector<ycge_ctx *> ctxs = contexts_of(c);
    for (ycge_ctx *x : ctxs) {          // room on every device first (contents kept), then the new records: nothing refers to them yet
        HIP_TRY(c, hipSetDevice(x->device));
        const size_t cap = x->d_materials.p ? x->d_materials.cap : 0;
        const hipError_t e = grow_preserve(x->d_materials, have + (size_t)n > cap ? std::max(have + (size_t)n, 2 * cap) : have + (size_t)n, have);
        x->sd.materials = x->d_materials.p;
        HIP_TRY(c, e);
    }
    for (ycge_ctx *x : ctxs) {
        HIP_TRY(c, hipSetDevice(x->device));
        HIP_TRY(c, hipMemcpy(x->d_materials.p + have, mats.data(), (size_t)n * sizeof(GMaterial), hipMemcpyHostToDevice));
    }
    // ---- nothing below fails
    for (ycge_ctx *x : ctxs) {
        x->d_materials.n = have + (size_t)n;
        x->n_materials = (int)have + n;
        if (can_mirror) x->materials_can_mirror = true;
    }
    c->pending_transparent |= transparent; c->pending_textured |= textured;
    *out_first_index = (int32_t)have;
    return YCGE_OK;
}

int mesh_pool_stats(ycge_ctx *c, int64_t *out12)
{
    const MeshPool &P = c->mesh_pool;
    out12[0] = P.n_resident; out12[1] = (int64_t)P.ranges.free_index.size(); out12[2] = P.units_in_use;
    out12[3] = (int64_t)(P.pooled ? P.capacity : P.ranges.end); out12[4] = P.growths; out12[5] = P.ranges.ranges_reused;
    out12[6] = P.device_builds; out12[7] = P.host_builds;
    for (int a = 0; a < 3; a++) out12[8 + a] = (int64_t)P.last_attach_us[a];
    out12[11] = P.pooled ? 1 : 0;
    return YCGE_OK;
}

}  // namespace ycge_host
