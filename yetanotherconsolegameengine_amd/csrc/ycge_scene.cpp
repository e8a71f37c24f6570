// ycge_scene.cpp - the scene on the host side of the C-ABI: argument checks, flattening (materials, textures, grids, Scene.Objects and
// the scene BVH), ycge_scene_upload as a list of named steps over SceneArrays, the installs on every device, and the scene updates
// (lights, a live texture's frame, objects).  The mesh trees and the mesh arena the upload asks for: ycge_mesh_bvh.cpp.  Streamed grids:
// ycge_grid_encode.cpp.
#include "ycge_ctx.h"

namespace ycge_host {

// Hittable.TryGetBounds of each primitive class (see the citations in include/ycge.h)
bool prim_bounds(const ycge_prim &q, const std::vector<MeshHost> &meshes, const std::vector<std::array<float, 6>> &grid_bounds, float b[6], float cen[3])
{
    const float *p = q.p;
    const float eps = 1e-4f;
    bool from_box = true;
    switch (q.type) {
    case YCGE_PRIM_SPHERE:
        b[0] = p[0] - p[3]; b[1] = p[1] - p[3]; b[2] = p[2] - p[3]; b[3] = p[0] + p[3]; b[4] = p[1] + p[3]; b[5] = p[2] + p[3]; break;
    case YCGE_PRIM_PLANE:
        b[0] = b[1] = b[2] = -1e6f; b[3] = b[4] = b[5] = 1e6f; cen[0] = cen[1] = cen[2] = 0.0f; from_box = false; break;
    case YCGE_PRIM_DISK:
        b[0] = p[0] - p[6]; b[1] = p[1] - p[6]; b[2] = p[2] - p[6]; b[3] = p[0] + p[6]; b[4] = p[1] + p[6]; b[5] = p[2] + p[6]; break;
    case YCGE_PRIM_XYRECT: b[0] = p[0]; b[1] = p[2]; b[2] = p[4] - eps; b[3] = p[1]; b[4] = p[3]; b[5] = p[4] + eps; break;
    case YCGE_PRIM_XZRECT: b[0] = p[0]; b[1] = p[4] - eps; b[2] = p[2]; b[3] = p[1]; b[4] = p[4] + eps; b[5] = p[3]; break;
    case YCGE_PRIM_YZRECT: b[0] = p[4] - eps; b[1] = p[0]; b[2] = p[2]; b[3] = p[4] + eps; b[4] = p[1]; b[5] = p[3]; break;
    case YCGE_PRIM_BOX: for (int k = 0; k < 6; k++) b[k] = p[k]; break;
    case YCGE_PRIM_CYLINDER_Y:
        b[0] = p[0] - p[3]; b[1] = cs_min(p[4], p[5]); b[2] = p[2] - p[3]; b[3] = p[0] + p[3]; b[4] = cs_max(p[4], p[5]); b[5] = p[2] + p[3]; break;
    case YCGE_PRIM_TRIANGLE:
        for (int a = 0; a < 3; a++) {
            b[a] = cs_min(p[a], cs_min(p[3 + a], p[6 + a])) - eps;
            b[3 + a] = cs_max(p[a], cs_max(p[3 + a], p[6 + a])) + eps;
        }
        break;
    case YCGE_PRIM_MESH: {
        const BuiltTree &t = meshes[q.ref].tree;
        if (t.root < 0) return false;
        const RefNode &r = t.nodes[t.root];
        for (int a = 0; a < 3; a++) { b[a] = r.mn[a]; b[3 + a] = r.mx[a]; }
        break;
    }
    case YCGE_PRIM_VOLUME_GRID: {
        const std::array<float, 6> &gb = grid_bounds[q.ref];
        if (!(gb[3] >= gb[0])) return false;                 // empty grid (marked at upload)
        for (int k = 0; k < 6; k++) b[k] = gb[k];
        break;
    }
    default: return false;
    }
    if (from_box) for (int a = 0; a < 3; a++) cen[a] = 0.5f * (b[a] + b[3 + a]);
    return true;
}

static int upload_lights(ycge_ctx *c, const ycge_light *lights, int n)
{
    std::vector<GLight> L(n);
    c->any_light_lit = false;
    for (int i = 0; i < n; i++) {
        L[i].pos[0] = lights[i].position.x; L[i].pos[1] = lights[i].position.y; L[i].pos[2] = lights[i].position.z;
        L[i].color[0] = lights[i].color.x; L[i].color[1] = lights[i].color.y; L[i].color[2] = lights[i].color.z;
        L[i].intensity = lights[i].intensity;
        L[i].dark = (lights[i].intensity == 0.0f && std::isfinite(lights[i].color.x) && std::isfinite(lights[i].color.y) && std::isfinite(lights[i].color.z)) ? 1.0f : 0.0f;
        if (L[i].dark == 0.0f) c->any_light_lit = true;
    }
    HIP_TRY(c, c->d_lights.upload(L));
    c->sd.lights = c->d_lights.p;
    c->sd.n_lights = n;
    return YCGE_OK;
}

// ---- one ycge_grid: the argument checks and the host arithmetic of its record, shared by ycge_scene_upload and ycge_scene_attach_grids
int validate_grid(const ycge_grid &g, int gi, int n_materials, std::string &msg)
{
    char buf[256];
    auto bad = [&](int code, const char *fmt, int a = 0, int b = 0) { std::snprintf(buf, sizeof buf, fmt, a, b); msg = buf; return code; };
    if (g.nx <= 0 || g.ny <= 0 || g.nz <= 0 || !g.cells) return bad(YCGE_ERR_INVALID_ARG, "grid %d: empty", gi);
    if ((uint64_t)g.nx * g.ny * g.nz >= (1u << 30)) return bad(YCGE_ERR_UNSUPPORTED, "grid %d: more than 2^30 cells", gi);
    // (the voxel walk forms brick indices with 24-bit multiplies: ((z >> 3) * bricks_y + (y >> 3)) * bricks_x)
    if ((uint64_t)((g.nz + 7) >> 3) * (uint64_t)((g.ny + 7) >> 3) >= (1u << 23) || ((g.nx + 7) >> 3) >= (1 << 23))
        return bad(YCGE_ERR_UNSUPPORTED, "grid %d: more than 2^23 bricks across one face", gi);
    if (g.n_lookup < 0 || (g.n_lookup > 0 && !g.lookup)) return bad(YCGE_ERR_INVALID_ARG, "grid %d: bad lookup table", gi);
    for (int k = 0; k < g.n_lookup; k++)
        if (g.lookup[k].material < 0 || g.lookup[k].material >= n_materials) return bad(YCGE_ERR_INVALID_ARG, "grid %d: lookup entry %d names a material out of range", gi, k);
    return YCGE_OK;
}

// the record's fields that come from the arguments alone (VolumeGrid ctor, VolumeGrid.cs:55-93); cell_offset, lut_offset and the solid box follow
void grid_record_init(const ycge_grid &g, GGrid &G)
{
    std::memset(&G, 0, sizeof G);
    G.nx = g.nx; G.ny = g.ny; G.nz = g.nz;
    G.nbx = (g.nx + 7) >> 3; G.nby = (g.ny + 7) >> 3; G.nbz = (g.nz + 7) >> 3;
    G.min_corner[0] = g.min_corner.x; G.min_corner[1] = g.min_corner.y; G.min_corner[2] = g.min_corner.z;
    G.voxel_size[0] = cs_max(1e-6f, g.voxel_size.x); G.voxel_size[1] = cs_max(1e-6f, g.voxel_size.y); G.voxel_size[2] = cs_max(1e-6f, g.voxel_size.z);
    G.wireframe = g.wireframe ? 1 : 0;
    float ww = g.wire_width_fraction; if (ww < 0.0f) ww = 0.0f; if (ww > 0.5f) ww = 0.5f;
    G.wire_width_frac = ww;
    float wm = g.wire_max_distance; if (wm < 0.0f) wm = 0.0f;
    G.wire_max_distance = wm;
    // How far along a ray the one-voxel margin of the solid box is provably enough.  The reference's walk reaches a cell by repeated
    // binary32 additions to tMax (VolumeGrid.cs:205-226): after k steps its t is off by at most k * ulp(t) / 2, i.e. the cell path
    // may drift k * t * 2^-24 world units from the true ray, with k <= nx + ny + nz steps inside one grid.  The cull (and the early
    // end of a walk at the box's exit) assumes that drift stays below HALF a voxel: t <= voxel * 2^23 / (nx + ny + nz) - 87 000 voxel
    // lengths for a 32^3 chunk; half of that is what is stored.  Beyond it the timed kernels walk the grid as the reference does.
    const float vs = cs_min(G.voxel_size[0], cs_min(G.voxel_size[1], G.voxel_size[2]));
    G.cull_t_limit = vs * 4194304.0f / (float)(G.nx + G.ny + G.nz);
    G.has_brick_mask = (size_t)G.nbx * G.nby * G.nbz <= 64 ? 1 : 0;
}

// ... and those that come from the cells: the index box lo..hi of the solid voxels (hi < 0: none) and the brick mask
void grid_record_solid(GGrid &G, const int lo[3], const int hi[3], uint64_t brick_mask)
{
    for (int a = 0; a < 3; a++) {           // one voxel of margin on every side (GGrid::solid_lo / solid_hi)
        G.solid_lo[a] = hi[a] < 0 ? 1.0f : G.min_corner[a] + (float)(lo[a] - 1) * G.voxel_size[a];
        G.solid_hi[a] = hi[a] < 0 ? 0.0f : G.min_corner[a] + (float)(hi[a] + 2) * G.voxel_size[a];
    }
    G.brick_mask_lo = (uint32_t)brick_mask; G.brick_mask_hi = (uint32_t)(brick_mask >> 32);
}

std::array<float, 6> grid_world_bounds(const ycge_grid &g)          // VolumeGrid.TryGetBounds, VolumeGrid.cs:95-97
{
    const float vs[3] = {cs_max(1e-6f, g.voxel_size.x), cs_max(1e-6f, g.voxel_size.y), cs_max(1e-6f, g.voxel_size.z)};
    return {{g.min_corner.x, g.min_corner.y, g.min_corner.z, g.min_corner.x + (float)g.nx * vs[0], g.min_corner.y + (float)g.ny * vs[1],
             g.min_corner.z + (float)g.nz * vs[2]}};
}

// The host encoder: one byte per voxel = index into a per-grid material table.  `cells` = the grid's nbx * nby * nbz * 512 zeroed bytes,
// `lut` receives the table (entry 0 = -1: empty; codes 1.. = distinct (matId, metaId) pairs in first-seen order, at most 255).
int encode_grid_host(ycge_ctx *c, const ycge_grid &g, int gi, int n_materials, const GGrid &G, uint8_t *cells, std::vector<int32_t> &lut, int lo[3], int hi[3],
                     uint64_t &brick_mask, std::vector<std::pair<int32_t, int32_t>> *seen_out)
{
    auto mat_ok = [&](int mi) { return mi >= 0 && mi < n_materials; };
    std::vector<std::pair<int32_t, int32_t>> own;
    std::vector<std::pair<int32_t, int32_t>> &seen = seen_out ? *seen_out : own;
    seen.clear();
    lut.push_back(-1);
    const bool maskable = G.has_brick_mask != 0;
    brick_mask = 0;
    lo[0] = g.nx; lo[1] = g.ny; lo[2] = g.nz; hi[0] = hi[1] = hi[2] = -1;          // index box of the solid voxels
    for (int iz = 0; iz < g.nz; iz++)
        for (int iy = 0; iy < g.ny; iy++)
            for (int ix = 0; ix < g.nx; ix++) {
                const size_t src = ((size_t)ix * g.ny + iy) * g.nz + iz;
                const int32_t mat = g.cells[2 * src], meta = g.cells[2 * src + 1];
                if (mat <= 0) continue;
                int code = -1;
                for (size_t k = 0; k < seen.size(); k++) if (seen[k].first == mat && seen[k].second == meta) { code = (int)k + 1; break; }
                if (code < 0) {
                    if (seen.size() >= 255) return c->fail(YCGE_ERR_UNSUPPORTED, "grid %d: more than 255 distinct (matId, metaId) pairs", gi);
                    int material = g.default_material;
                    for (int k = 0; k < g.n_lookup; k++) if (g.lookup[k].mat_id == mat && g.lookup[k].meta_id == meta) { material = g.lookup[k].material; break; }
                    if (!mat_ok(material)) return c->fail(YCGE_ERR_INVALID_ARG, "grid %d: no material for (matId %d, metaId %d)", gi, mat, meta);
                    seen.push_back({mat, meta});
                    lut.push_back(material);
                    code = (int)seen.size();
                }
                const int brick = (((iz >> 3) * G.nby) + (iy >> 3)) * G.nbx + (ix >> 3);
                cells[(size_t)brick * 512 + morton3(ix & 7, iy & 7, iz & 7)] = (uint8_t)code;
                if (maskable) brick_mask |= (uint64_t)1 << brick;
                if (ix < lo[0]) lo[0] = ix; if (ix > hi[0]) hi[0] = ix;
                if (iy < lo[1]) lo[1] = iy; if (iy > hi[1]) hi[1] = iy;
                if (iz < lo[2]) lo[2] = iz; if (iz > hi[2]) hi[2] = iz;
            }
    return YCGE_OK;
}

// ---- argument checks of ycge_scene_upload (pure host code; also exported as ycge_validate_scene)
int validate_scene(const ycge_scene *s, std::string &msg)
{
    char buf[256];
    auto bad = [&](int code, const char *fmt, int a = 0, int b = 0, int c2 = 0) { std::snprintf(buf, sizeof buf, fmt, a, b, c2); msg = buf; return code; };
    if (!s) return bad(YCGE_ERR_INVALID_ARG, "null scene");
    if (s->n_prims < 0 || s->n_materials < 0 || s->n_lights < 0 || s->n_meshes < 0 || s->n_grids < 0) return bad(YCGE_ERR_INVALID_ARG, "negative count");
    if ((s->n_prims > 0 && !s->prims) || (s->n_materials > 0 && !s->materials) || (s->n_lights > 0 && !s->lights) || (s->n_meshes > 0 && !s->meshes) ||
        (s->n_grids > 0 && !s->grids))
        return bad(YCGE_ERR_INVALID_ARG, "null array with a non-zero count");
    auto mat_ok = [&](int mi) { return mi >= 0 && mi < s->n_materials; };
    for (int i = 0; i < s->n_materials; i++) {
        const int k = s->materials[i].kind;
        if (k == YCGE_MAT_TEXTURED) {
            if (s->materials[i].texture < 0 || s->materials[i].texture >= s->n_textures)
                return bad(YCGE_ERR_INVALID_ARG, "material %d: texture index %d out of range (%d textures)", i, s->materials[i].texture, s->n_textures);
        } else if (k != YCGE_MAT_CONSTANT && k != YCGE_MAT_CHECKER) return bad(YCGE_ERR_UNSUPPORTED, "material %d: unknown kind %d", i, k);
    }
    if (s->n_textures < 0 || (s->n_textures > 0 && !s->textures)) return bad(YCGE_ERR_INVALID_ARG, "bad texture array");
    for (int i = 0; i < s->n_textures; i++) {
        const ycge_texture &t = s->textures[i];
        if (t.frame_bytes_per_pixel != 0 && t.frame_bytes_per_pixel != 3 && t.frame_bytes_per_pixel != 4) return bad(YCGE_ERR_INVALID_ARG, "texture %d: frame_bytes_per_pixel %d (0 static, 3 BGR, 4 BGRA)", i, t.frame_bytes_per_pixel);
        if (t.width < 1 || t.height < 1 || (!t.pixels && t.frame_bytes_per_pixel == 0)) return bad(YCGE_ERR_INVALID_ARG, "texture %d: needs width, height >= 1 and pixels (%d x %d)", i, t.width, t.height);
        if ((long long)t.width * t.height > (1ll << 28)) return bad(YCGE_ERR_UNSUPPORTED, "texture %d: above 2^28 pixels", i);
    }
    for (int mi = 0; mi < s->n_meshes; mi++) {
        const ycge_mesh &m = s->meshes[mi];
        if (m.n_triangles < 0 || (m.n_triangles > 0 && !m.triangles)) return bad(YCGE_ERR_INVALID_ARG, "mesh %d: bad triangle array", mi);
        if (!m.tri_material && !mat_ok(m.material)) return bad(YCGE_ERR_INVALID_ARG, "mesh %d: material out of range", mi);
        if (m.tri_material)
            for (int t = 0; t < m.n_triangles; t++)
                if (!mat_ok(m.tri_material[t])) return mesh_refusal(MESH_TRI_MATERIAL, mi, msg);
    }
    for (int gi = 0; gi < s->n_grids; gi++) {
        const int rc = validate_grid(s->grids[gi], gi, s->n_materials, msg);
        if (rc != YCGE_OK) return rc;
    }
    for (int i = 0; i < s->n_prims; i++) {
        const ycge_prim &q = s->prims[i];
        if (q.type < YCGE_PRIM_SPHERE || q.type > YCGE_PRIM_VOLUME_GRID) return bad(YCGE_ERR_INVALID_ARG, "prim %d: unknown type %d", i, q.type);
        if (q.type == YCGE_PRIM_MESH) { if (q.ref < 0 || q.ref >= s->n_meshes) return bad(YCGE_ERR_INVALID_ARG, "prim %d: mesh ref out of range", i); }
        else if (q.type == YCGE_PRIM_VOLUME_GRID) { if (q.ref < 0 || q.ref >= s->n_grids) return bad(YCGE_ERR_INVALID_ARG, "prim %d: grid ref out of range", i); }
        else if (!mat_ok(q.material)) return bad(YCGE_ERR_INVALID_ARG, "prim %d: material out of range", i);
    }
    return YCGE_OK;
}

// Scene.Objects -> object records + scene BVH (BVH ctor, BVH.cs:29-97), built on the host ONCE per update (rank 0's context
// keeps the metadata of the last full upload: mesh root boxes, grid bounds, material count) and installed on every device.
struct ObjectsHost {
    std::vector<GPrim> gprims;
    std::vector<GNode> scene_nodes;
    std::vector<uint32_t> leaf_prims;
    uint32_t scene_root = YCGE_REF_NONE_VALUE;
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};
    int wf_rounds = 2, spill_levels = 0;
    std::vector<int32_t> grid_owner;       // per grid of the last upload: the object that holds it (-1: none), SceneDev::grid_owner
    bool grid_owner_unique = true;         // false: two objects hold the same grid - no walk tree
    bool any_grid_object = false;          // some object of the list IS a voxel grid (the scene's grid TABLE may hold grids no object uses: their entity left)
    float walk_t_limit = 0.0f;             // the smallest GGrid::cull_t_limit of the grids in Objects
    bool analytic_only = true;             // no mesh and no voxel grid among the objects (SceneDev::analytic_only)
};

// Scene.Objects as device records + what Scene.RebuildBVH gets from every object's TryGetBounds (BVH.cs:32-53); no tree yet
int flatten_objects(ycge_ctx *c, const ycge_prim *prims, int n_prims, ObjectsHost &oh, BoundsSoA &items)
{
    std::vector<GPrim> &gprims = oh.gprims;
    gprims.assign(n_prims, GPrim{});
    items.resize(n_prims);
    oh.grid_owner.assign(c->grid_solid.size(), -1); oh.grid_owner_unique = true; oh.any_grid_object = false; oh.walk_t_limit = HUGE_VALF;
    oh.analytic_only = true;
    for (int i = 0; i < n_prims; i++) {
        const ycge_prim &q = prims[i];
        if (q.type == YCGE_PRIM_MESH || q.type == YCGE_PRIM_VOLUME_GRID) oh.analytic_only = false;
        GPrim &g = gprims[i];
        std::memset(&g, 0, sizeof g);
        g.type = q.type; g.material = q.material; g.ref = q.ref; g.reflectivity = q.reflectivity;
        const float *p = q.p;
        switch (q.type) {
        case YCGE_PRIM_SPHERE: for (int k = 0; k < 4; k++) g.p[k] = p[k]; break;
        case YCGE_PRIM_PLANE: {      // Plane ctor, Surfaces.cs:19-28
            H3 n = h_norm(H3{p[3], p[4], p[5]});
            g.p[0] = n.x; g.p[1] = n.y; g.p[2] = n.z;
            g.p[3] = n.x * p[0] + n.y * p[1] + n.z * p[2];
            break;
        }
        case YCGE_PRIM_DISK: {       // Disk ctor, Surfaces.cs:84-94
            H3 n = h_norm(H3{p[3], p[4], p[5]});
            g.p[0] = p[0]; g.p[1] = p[1]; g.p[2] = p[2]; g.p[3] = n.x; g.p[4] = n.y; g.p[5] = n.z;
            g.p[6] = p[6] * p[6];
            g.p[7] = n.x * p[0] + n.y * p[1] + n.z * p[2];
            break;
        }
        case YCGE_PRIM_XYRECT: case YCGE_PRIM_XZRECT: case YCGE_PRIM_YZRECT: for (int k = 0; k < 5; k++) g.p[k] = p[k]; break;
        case YCGE_PRIM_BOX: for (int k = 0; k < 6; k++) g.p[k] = p[k]; break;
        case YCGE_PRIM_CYLINDER_Y:   // CylinderY ctor, BoundedObjects.cs:128-137
            g.p[0] = p[0]; g.p[1] = p[2]; g.p[2] = p[3]; g.p[3] = p[3] * p[3];
            g.p[4] = cs_min(p[4], p[5]); g.p[5] = cs_max(p[4], p[5]); g.p[6] = p[6];
            break;
        case YCGE_PRIM_TRIANGLE: {   // Triangle ctor, Triangle.cs:36-45
            float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
            float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
            float nnx = e1y * e2z - e1z * e2y, nny = e1z * e2x - e1x * e2z, nnz = e1x * e2y - e1y * e2x;
            float inv_len = 1.0f / cs_max(1e-20f, cs_sqrt(nnx * nnx + nny * nny + nnz * nnz));
            g.p[0] = p[0]; g.p[1] = p[1]; g.p[2] = p[2];
            g.p[3] = e1x; g.p[4] = e1y; g.p[5] = e1z; g.p[6] = e2x; g.p[7] = e2y; g.p[8] = e2z;
            g.p[9] = nnx * inv_len; g.p[10] = nny * inv_len; g.p[11] = nnz * inv_len;
            break;
        }
        case YCGE_PRIM_MESH: {      // root box + root reference ride in the object record (one fetch less per query)
            if (q.ref < 0 || q.ref >= (int)c->gmeshes_host.size()) return c->fail(YCGE_ERR_INVALID_ARG, "prim %d: mesh ref out of range", i);
            const GMesh &gm = c->gmeshes_host[q.ref];
            for (int a = 0; a < 3; a++) { g.p[a] = gm.root_min[a]; g.p[3 + a] = gm.root_max[a]; }
            g.p[6] = u2f(gm.root_ref);
            break;
        }
        case YCGE_PRIM_VOLUME_GRID:
            if (q.ref < 0 || q.ref >= (int)c->grid_bounds.size() || !c->grid_pool.resident[(size_t)q.ref]) return c->fail(YCGE_ERR_INVALID_ARG, "prim %d: grid ref out of range", i);
            for (int k = 0; k < 7; k++) g.p[k] = c->grid_solid[q.ref][k];       // box of the grid's solid voxels + how far along a ray it may be trusted (grid_cull in the walk)
            if (oh.grid_owner[(size_t)q.ref] >= 0) oh.grid_owner_unique = false;
            oh.grid_owner[(size_t)q.ref] = i;
            oh.any_grid_object = true;
            oh.walk_t_limit = cs_min(oh.walk_t_limit, c->grid_solid[q.ref][6]);
            break;
        default: return c->fail(YCGE_ERR_INVALID_ARG, "prim %d: unknown type %d", i, q.type);
        }
        if (q.type != YCGE_PRIM_MESH && q.type != YCGE_PRIM_VOLUME_GRID && !(q.material >= 0 && q.material < c->n_materials))
            return c->fail(YCGE_ERR_INVALID_ARG, "prim %d: material out of range", i);
        float b[6], cen[3];
        if (!prim_bounds(q, c->meshes, c->grid_bounds, b, cen)) return c->fail(YCGE_ERR_INVALID_ARG, "Unbounded Hittable (prim %d)", i);   // BVH.cs:37-40
        for (int a = 0; a < 3; a++) { items.mn[a][i] = b[a]; items.mx[a][i] = b[3 + a]; items.c[a][i] = cen[a]; }
    }
    // can any surface take the mirror branch (Reflectivity >= MirrorThreshold, RaytraceRenderer.cs:559)?
    bool can_mirror = c->materials_can_mirror;
    for (int i = 0; i < n_prims; i++) {
        const int ty = prims[i].type;
        const bool overrides = ty == YCGE_PRIM_PLANE || ty == YCGE_PRIM_DISK || ty == YCGE_PRIM_XYRECT || ty == YCGE_PRIM_XZRECT || ty == YCGE_PRIM_YZRECT || ty == YCGE_PRIM_BOX;
        if (overrides && prims[i].reflectivity >= c->cfg.mirror_threshold) can_mirror = true;
    }
    oh.wf_rounds = can_mirror ? 2 + c->cfg.max_mirror_bounces : 2;
    return YCGE_OK;
}

int check_scene_depth(ycge_ctx *c, int max_depth, int &spill_levels)
{
    // (the mesh trees are built once, by the root context: a peer's own max_mesh_depth mirrors it - install_scene - and the root's is what counts)
    const int mesh_depth = c->parent ? c->parent->max_mesh_depth : c->max_mesh_depth;
    if (max_depth > 128) return c->fail(YCGE_ERR_STACK_DEPTH, "scene BVH depth %d exceeds the reference's 128-entry stack (BVH.cs:118)", max_depth);
    if (max_depth + 4 + mesh_depth + 2 > YCGE_TRAVERSAL_STACK)
        return c->fail(YCGE_ERR_STACK_DEPTH, "combined traversal depth %d + %d exceeds the device stack", max_depth, mesh_depth);
    // levels the per-lane stack can need beyond its LDS part: scene depth + 4 leaf objects + deepest mesh
    const int need = max_depth + 4 + mesh_depth + 2 - YCGE_LDS_STACK_LEVELS;
    spill_levels = need > 0 ? need : 0;
    return YCGE_OK;
}

// the scene-level BVH by the host builder (ycge_accel.cpp)
int build_scene_tree_host(ycge_ctx *c, const BoundsSoA &items, ObjectsHost &oh)
{
    build_tree(items, TreeFlavour::Scene, c->scene_tree);
    c->scene_tree_on_device = false;
    c->bvh_host_builds++;
    const int rc = check_scene_depth(c, c->scene_tree.max_depth, oh.spill_levels);
    if (rc != YCGE_OK) return rc;
    oh.scene_root = to_gpu_nodes(c->scene_tree, REF_SCENE_NODE, REF_SCENE_LEAF, 0, 0, 3, oh.scene_nodes);
    oh.leaf_prims.assign(c->scene_tree.leaf_index.begin(), c->scene_tree.leaf_index.end());
    if (c->scene_tree.root >= 0)
        for (int a = 0; a < 3; a++) { oh.root_min[a] = c->scene_tree.nodes[c->scene_tree.root].mn[a]; oh.root_max[a] = c->scene_tree.nodes[c->scene_tree.root].mx[a]; }
    return YCGE_OK;
}

// SceneDev::walk_nodes: the walk tree of a world of voxel grids, from the tree and the object records now on the device (k_scene_walk,
// ycge_bvh_build.hip) - whichever builder made the tree.  None (null) without a grid, when the root is a leaf, when two objects hold
// the same grid (grid_owner would be ambiguous), when NO object holds a grid although the scene's table has some (every voxel entity left
// through ycge_scene_update_objects, or the upload listed grids nothing uses: the objects are then analytic_only, and a walk tree beside
// that flag sent the timed k_trace out of bounds - a GPU memory fault found by the drawn call sequences of round 6) and under YCGE_NO_WALK_TREE.
int install_walk_tree(ycge_ctx *c, const ObjectsHost &oh, int n_inner, uint32_t scene_root)
{
    SceneDev &sd = c->sd;
    sd.walk_nodes = nullptr; sd.grid_owner = nullptr; sd.walk_root_ref = YCGE_REF_NONE_VALUE; sd.walk_t_limit = 0.0f; c->walk_scene_nodes = 0;
    if (!c->has_grid || !oh.any_grid_object || n_inner <= 0 || c->knobs.no_walk_tree || !oh.grid_owner_unique || YCGE_REF_KIND(scene_root) != REF_SCENE_NODE) return YCGE_OK;
    HIP_TRY(c, c->d_grid_owner.upload(oh.grid_owner));
    const size_t n_walk = (size_t)n_inner * (1 + 2 * YCGE_WALK_LEAF_NODES);
    HIP_TRY(c, c->d_walk_nodes.reserve(n_walk));
    HIP_TRY(c, hipMemsetAsync(c->d_walk_nodes.p, 0, n_walk * sizeof(GNode), c->stream));
    const int e = ycge_launch_scene_walk(c->d_scene_nodes.p, n_inner, c->d_scene_leaf.p, c->d_prims.p, c->d_walk_nodes.p, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_scene_walk launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    sd.walk_nodes = c->d_walk_nodes.p; sd.grid_owner = c->d_grid_owner.p;
    sd.walk_root_ref = YCGE_REF(REF_WALK_NODE, YCGE_REF_PAYLOAD(scene_root));
    sd.walk_t_limit = oh.walk_t_limit;
    c->walk_scene_nodes = n_inner;
    return YCGE_OK;
}

// What both object installs end with, once the records and the tree are in d_prims / d_scene_nodes / d_scene_leaf: the rounds of the
// wavefront path, the spill columns for the tree's depth, the scene's pointers and root, a new schedule, the walk tree.
int install_object_tree(ycge_ctx *c, const ObjectsHost &oh, uint32_t root_ref, const float root_min[3], const float root_max[3], int n_inner, int spill_levels)
{
    c->wf_rounds = oh.wf_rounds;
    if (spill_levels != c->spill_levels) {
        c->spill_levels = spill_levels;
        const int rc = alloc_tile_buffers(c);
        if (rc != YCGE_OK) return rc;
    }
    SceneDev &sd = c->sd;
    sd.scene_nodes = c->d_scene_nodes.p; sd.scene_leaf_prims = c->d_scene_leaf.p; sd.prims = c->d_prims.p;
    sd.scene_root_ref = root_ref;
    sd.analytic_only = (oh.analytic_only && !c->knobs.no_analytic_walk) ? 1 : 0;
    for (int a = 0; a < 3; a++) { sd.scene_root_min[a] = root_min[a]; sd.scene_root_max[a] = root_max[a]; }
    c->block_order_valid = false;
    return install_walk_tree(c, oh, n_inner, root_ref);
}

int install_objects(ycge_ctx *c, const ObjectsHost &oh)
{
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_prims.upload(oh.gprims)); HIP_TRY(c, c->d_scene_nodes.upload(oh.scene_nodes)); HIP_TRY(c, c->d_scene_leaf.upload(oh.leaf_prims));
    // (only this install forgets which frame each schedule in flight was built for; install_objects_device_built does not, and nothing
    // records why: unexplained, kept as it is)
    c->flight_order_frame[0] = c->flight_order_frame[1] = c->flight_order_frame[2] = -1;
    return install_object_tree(c, oh, oh.scene_root, oh.root_min, oh.root_max, (int)oh.scene_nodes.size(), oh.spill_levels);
}

int build_objects(ycge_ctx *c, const ycge_prim *prims, int n_prims, ObjectsHost &oh)
{
    BoundsSoA items;
    const int rc = flatten_objects(c, prims, n_prims, oh, items);
    return rc != YCGE_OK ? rc : build_scene_tree_host(c, items, oh);
}

// ycge_scene_update_objects, device form: the object records and their boxes go up, ycge_bvh_build.hip builds the tree where the
// trace reads it.  Returns 1 when the kernel declines (a tree deeper than the reference's stack; the caller then builds on the host).
int install_objects_device_built(ycge_ctx *c, ycge_ctx *root, const ObjectsHost &oh, const BoundsSoA &items)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const int n = (int)items.size();
    std::vector<float> planes((size_t)9 * n);
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < n; i++) {
            planes[(size_t)a * n + i] = items.mn[a][i]; planes[(size_t)(3 + a) * n + i] = items.mx[a][i]; planes[(size_t)(6 + a) * n + i] = items.c[a][i];
        }
    HIP_TRY(c, c->d_prims.upload(oh.gprims)); HIP_TRY(c, c->d_bvh_items.upload(planes));
    HIP_TRY(c, c->d_scene_nodes.reserve((size_t)n)); HIP_TRY(c, c->d_scene_leaf.reserve((size_t)n));
    HIP_TRY(c, c->d_bvh_scratch.reserve(ycge_bvh_build_scratch_bytes(n))); HIP_TRY(c, c->d_bvh_ref.reserve((size_t)2 * n * sizeof(RefNode)));
    HIP_TRY(c, c->d_bvh_res.reserve(sizeof(BvhBuildResult)));
    const int e = ycge_launch_scene_bvh_build(c->d_bvh_items.p, n, c->d_bvh_scratch.p, c->d_bvh_ref.p, c->d_scene_nodes.p, c->d_scene_leaf.p, c->d_bvh_res.p, c->knobs.bvh_waves, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_scene_bvh_build launch failed: %s", hipGetErrorString((hipError_t)e));
    BvhBuildResult res;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    { const int cr = copy_out(c, &res, c->d_bvh_res.p, sizeof res); if (cr != YCGE_OK) return cr; }       // (through the library's page-locked staging: the device writes no caller or stack memory)
    if (res.fallback) return 1;
    int spill = 0;
    const int rc = check_scene_depth(c, res.max_depth, spill);
    if (rc != YCGE_OK) return rc;
    const int rc3 = install_object_tree(c, oh, res.root_ref, res.root_min, res.root_max, res.n_inner, spill);      // (flight_order_frame[] stays: see install_objects)
    if (rc3 != YCGE_OK) return rc3;
    if (c == root) { c->scene_tree_on_device = true; c->dev_tree_nodes = res.n_nodes; c->dev_tree_items = n; c->scene_tree.max_depth = res.max_depth; c->scene_tree.sort_fallbacks = (int32_t)res.sorts; }
    return YCGE_OK;
}

// the arrays of a full upload, built once and installed on every device
struct SceneArrays {
    std::vector<GMaterial> mats;
    std::vector<uint8_t> arena, cells;
    std::vector<GMesh> gmeshes;
    std::vector<GGrid> ggrids;
    std::vector<int32_t> lut;
    std::vector<SlotCodes> codes;           // per grid, for the grid pool
    bool any_transparent = false, has_grid = false, any_textured = false;
    std::vector<uint32_t> tex_pixels;
    std::vector<int32_t> tex_info;          // per texture {first word, width, height, 0 | live-frame flags}
    uint32_t tl_offset = 0;          // treelet region of the arena (append_treelets), 0 = none
    const ycge_ctx *arena_on = nullptr;     // the arena was assembled on this context's device (its d_mesh_arena holds it, `arena` is empty): the others copy it from there
    int max_mesh_depth = 0;                 // the deepest mesh tree (check_scene_depth, once the upload is remembered)
};

int install_scene(ycge_ctx *c, const SceneArrays &A, const ObjectsHost &oh, const ycge_scene *s)
{
    HIP_TRY(c, hipSetDevice(c->device));
    c->have_scene = false;
    HIP_TRY(c, c->d_materials.upload(A.mats));
    if (!A.arena_on) HIP_TRY(c, c->d_mesh_arena.upload(A.arena));
    else if (c != A.arena_on) {
        const DevBuf<uint8_t> &src = A.arena_on->d_mesh_arena;
        HIP_TRY(c, c->d_mesh_arena.alloc(src.n));
        if (c->device == A.arena_on->device) HIP_TRY(c, hipMemcpy(c->d_mesh_arena.p, src.p, src.n, hipMemcpyDeviceToDevice));
        else HIP_TRY(c, hipMemcpyPeer(c->d_mesh_arena.p, c->device, src.p, A.arena_on->device, src.n));
    }
    HIP_TRY(c, c->d_meshes.upload(A.gmeshes)); HIP_TRY(c, c->d_grids.upload(A.ggrids)); HIP_TRY(c, c->d_cells.upload(A.cells));
    HIP_TRY(c, c->d_lut.upload(A.lut));
    HIP_TRY(c, c->d_tex_pixels.upload(A.tex_pixels)); HIP_TRY(c, c->d_tex_info.upload(A.tex_info));
    c->tex_info_host = A.tex_info;
    SceneDev &sd = c->sd;
    std::memset(&sd, 0, sizeof sd);
    sd.mesh_arena = c->d_mesh_arena.p;
    sd.materials = c->d_materials.p; sd.meshes = c->d_meshes.p; sd.grids = c->d_grids.p;
    sd.grid_cells = c->d_cells.p; sd.grid_lut = c->d_lut.p;
    sd.tex_pixels = c->d_tex_pixels.p; sd.tex_info = c->d_tex_info.p;
    c->has_grid = A.has_grid;
    int rc = install_objects(c, oh);
    if (rc != YCGE_OK) return rc;
    sd.ambient[0] = s->ambient_color.x; sd.ambient[1] = s->ambient_color.y; sd.ambient[2] = s->ambient_color.z;
    sd.ambient_intensity = s->ambient_intensity;
    sd.bg_top[0] = s->background_top.x; sd.bg_top[1] = s->background_top.y; sd.bg_top[2] = s->background_top.z;
    sd.bg_bottom[0] = s->background_bottom.x; sd.bg_bottom[1] = s->background_bottom.y; sd.bg_bottom[2] = s->background_bottom.z;
    sd.is_volume_scene = s->is_volume_scene ? 1 : 0;
    c->has_dynamic_textures = s->has_dynamic_textures != 0;
    sd.any_transparent = A.any_transparent ? 1 : 0;
    sd.any_textured = A.any_textured ? 1 : 0;
    sd.tl_offset = A.tl_offset;
    sd.anyhit_bfs = (uint32_t)c->knobs.bfs_rays;
    if (!c->dbg_counters.p) { HIP_TRY(c, c->dbg_counters.alloc(16 + 64 * 256)); HIP_TRY(c, hipMemset(c->dbg_counters.p, 0, (16 + 64 * 256) * sizeof(unsigned long long))); }
    sd.dbg_counters = c->dbg_counters.p;
    rc = upload_lights(c, s->lights, s->n_lights);
    if (rc != YCGE_OK) return rc;
    c->have_scene = true;
    c->block_order_valid = false; c->flight_order_frame[0] = c->flight_order_frame[1] = c->flight_order_frame[2] = -1;
    return YCGE_OK;
}

// ---- the steps of ycge_scene_upload, in its order: each fills its part of A (the last ones: of the root context) or fails with the error's text on c

void flatten_material(const ycge_material &m, GMaterial &g, bool &any_transparent, bool &any_textured)
{
    std::memset(&g, 0, sizeof g);
    g.kind = m.kind;
    g.albedo[0] = m.albedo.x; g.albedo[1] = m.albedo.y; g.albedo[2] = m.albedo.z;
    g.albedo_b[0] = m.albedo_b.x; g.albedo_b[1] = m.albedo_b.y; g.albedo_b[2] = m.albedo_b.z;
    g.checker_scale = m.checker_scale;
    g.reflectivity = m.reflectivity;
    g.emission[0] = m.emission.x; g.emission[1] = m.emission.y; g.emission[2] = m.emission.z;
    g.transparency = m.transparency; g.ior = m.index_of_refraction;
    g.trans_color[0] = m.transmission_color.x; g.trans_color[1] = m.transmission_color.y; g.trans_color[2] = m.transmission_color.z;
    if (m.transparency > 0.0f) any_transparent = true;
    g.tex = -1;
    if (m.kind == YCGE_MAT_TEXTURED && m.texture_weight > 0.0) {     // SampleAlbedo, RaytraceRenderer.cs:726-733 (a weight <= 0: the plain albedo)
        g.tex = m.texture;
        any_textured = true;
        g.tex_tiles = (float)(m.uv_scale > 1e-6 ? m.uv_scale : 1e-6);                                            // (float)Math.Max(1e-6, mat.UVScale)
        g.tex_t = (float)(m.texture_weight < 0.0 ? 0.0 : m.texture_weight > 1.0 ? 1.0 : m.texture_weight);       // (float)Math.Clamp(mat.TextureWeight, 0.0, 1.0)
    }
}

int flatten_materials(const ycge_scene *s, SceneArrays &A)
{
    A.mats.assign(s->n_materials, GMaterial{});
    for (int i = 0; i < s->n_materials; i++) flatten_material(s->materials[i], A.mats[i], A.any_transparent, A.any_textured);
    return YCGE_OK;
}

int flatten_textures(const ycge_scene *s, SceneArrays &A)
{
    for (int i = 0; i < s->n_textures; i++) {
        const ycge_texture &t = s->textures[i];
        // info.w: 0 = static (RGBA32 ints); else bytes per pixel of a live texture's frames | flipU << 4 | flipV << 5, the frame's bytes packed into words
        const int bpp = t.frame_bytes_per_pixel;
        const int32_t info[4] = {(int32_t)A.tex_pixels.size(), t.width, t.height, bpp ? (bpp | (t.flip_u ? 16 : 0) | (t.flip_v ? 32 : 0)) : 0};
        A.tex_info.insert(A.tex_info.end(), info, info + 4);
        if (!bpp) A.tex_pixels.insert(A.tex_pixels.end(), t.pixels, t.pixels + (size_t)t.width * t.height);
        else {
            const size_t nbytes = (size_t)t.width * t.height * bpp, nwords = (nbytes + 3) / 4;
            const size_t at = A.tex_pixels.size();
            A.tex_pixels.resize(at + nwords, 0u);
            if (t.frame) std::memcpy(A.tex_pixels.data() + at, t.frame, nbytes);
        }
    }
    return YCGE_OK;
}

// meshes: MeshBVH ctor (MeshBVH.cs:41-130) -> a tree per mesh (build_mesh_tree, ycge_mesh_bvh.cpp), then ONE arena of all of them: GNode (64 B)
// and GTriPair (96 B) records addressed in 32-byte units, the treelets behind them.  The device assembles the arena (ycge_mesh_emit.hip) when
// at least one tree of this upload was built there, of a mesh of YCGE_MESH_EMIT_DEVICE_MIN triangles or more; else the host writes it.
int build_mesh_arena(ycge_ctx *c, const ycge_scene *s, SceneArrays &A)
{
    const Knobs &k = c->knobs;
    MeshEmit &E = c->mesh_emit;
    MeshUploadScratch scratch_of_this_upload{c->mesh_bvh, E};
    c->meshes.assign(s->n_meshes, MeshHost{});
    c->mesh_pool = MeshPool{};          // (the pool describes c->meshes: nothing is resident until this upload is remembered)
    A.gmeshes.assign(s->n_meshes, GMesh{});
    c->mesh_bvh_sorts = c->mesh_bvh_depth = c->mesh_bvh_wide_nodes = c->mesh_bvh_jobs = 0;
    c->mesh_emit_dev_meshes = c->mesh_emit_host_meshes = c->mesh_emit_arena_bytes = 0; c->mesh_emit_last_us = 0.0;
    auto worth_the_device_emit = [&](const ycge_mesh &m) { return m.n_triangles >= 1 && m.n_triangles >= k.mesh_bvh_device_min && m.n_triangles >= k.mesh_emit_device_min; };
    bool device_emit_still_possible = false;          // the knobs allow it and the builder is offered a mesh worth it: trees built on the device are kept there
    if (!k.mesh_emit_host && !k.mesh_bvh_host)
        for (int mi = 0; mi < s->n_meshes; mi++) device_emit_still_possible |= worth_the_device_emit(s->meshes[mi]);

    // ---- the trees, every mesh
    for (int mi = 0; mi < s->n_meshes; mi++) {
        const ycge_mesh &m = s->meshes[mi];
        BuiltTree &t = c->meshes[mi].tree;
        bool on_device = false;
        MeshBvhReport rep;
        const int brc = build_mesh_tree(k, false, c->mesh_bvh, m.triangles, m.n_triangles, c->stream, t, on_device, rep);
        if (brc < 0) return c->fail(brc, "mesh %d: device-side BVH build failed: %s", mi, hipGetErrorString(rep.error));
        if (on_device) { c->mesh_bvh_device_builds++; c->mesh_bvh_last_us = rep.us; c->mesh_bvh_wide_nodes += rep.wide_nodes; c->mesh_bvh_jobs += rep.jobs; }
        else { c->mesh_bvh_host_builds++; c->mesh_bvh_host_fallbacks += rep.fallback != MESH_BVH_BUILT ? 1 : 0; }
        c->mesh_bvh_sorts += t.sort_fallbacks;
        if (t.max_depth > c->mesh_bvh_depth) c->mesh_bvh_depth = t.max_depth;
        if (t.max_depth > 64) return c->fail(YCGE_ERR_STACK_DEPTH, "mesh %d: BVH depth %d exceeds the reference's 64-entry stack (MeshBVH.cs:150)", mi, t.max_depth);
        if (t.max_depth > A.max_mesh_depth) A.max_mesh_depth = t.max_depth;
        GMesh &gm = A.gmeshes[mi];
        std::memset(&gm, 0, sizeof gm);
        if (t.root >= 0) for (int a = 0; a < 3; a++) { gm.root_min[a] = t.nodes[t.root].mn[a]; gm.root_max[a] = t.nodes[t.root].mx[a]; }
        // A tree built on the device is handed to the emit HERE, inside the loop: its triangles, nodes and leaf order are the builder's
        // scratch, and the next build takes that scratch for itself.
        if (device_emit_still_possible && on_device) HIP_TRY(c, mesh_emit_add(E, (size_t)mi, true, c->mesh_bvh, t, m.triangles, m.n_triangles, m.tri_material, m.material));
    }

    // ---- the arena, decided once: on the device when a mesh worth it was built there
    auto kept_on_device = [&](int mi) { return (size_t)mi < E.in.size() && E.in[(size_t)mi].ready; };
    bool on_the_device = false;
    for (int mi = 0; mi < s->n_meshes; mi++) on_the_device |= kept_on_device(mi) && worth_the_device_emit(s->meshes[mi]);
    std::string msg;
    if (!on_the_device) {
        const int erc = emit_arena_on_host(c->meshes, s->meshes, s->n_materials, k.no_coop, A.arena, A.gmeshes, A.tl_offset, msg);
        if (erc != YCGE_OK) return c->fail(erc, "%s", msg.c_str());
        c->mesh_emit_host_meshes = s->n_meshes;
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        for (int mi = 0; mi < s->n_meshes; mi++) {          // (the trees the host built go up beside the kept ones)
            const ycge_mesh &m = s->meshes[mi];
            if (!kept_on_device(mi)) HIP_TRY(c, mesh_emit_add(E, (size_t)mi, false, c->mesh_bvh, c->meshes[mi].tree, m.triangles, m.n_triangles, m.tri_material, m.material));
        }
        std::vector<uint32_t> root_refs;
        const int erc = emit_arena_on_device(E, c->mesh_bvh.stage, c->d_mesh_arena, s->n_materials, k.no_coop, false, c->stream, root_refs, A.tl_offset, msg);
        if (erc != YCGE_OK) return c->fail(erc, "%s", msg.c_str());
        for (int mi = 0; mi < s->n_meshes; mi++) A.gmeshes[mi].root_ref = root_refs[(size_t)mi];
        A.arena_on = c;
        c->mesh_emit_dev_meshes = s->n_meshes;
        c->mesh_emit_last_us = us_since(t0);
    }
    c->mesh_emit_arena_bytes = A.arena_on ? (int64_t)c->d_mesh_arena.n : (int64_t)A.arena.size();
    return YCGE_OK;
}

// voxel grids: VolumeGrid ctor (VolumeGrid.cs:55-93), one byte per voxel = index into a per-grid material table
int encode_grids(ycge_ctx *c, const ycge_scene *s, SceneArrays &A)
{
    std::vector<GGrid> &ggrids = A.ggrids;
    ggrids.assign(s->n_grids, GGrid{});
    std::vector<uint8_t> &cells = A.cells;
    std::vector<int32_t> &lut = A.lut;
    for (int gi = 0; gi < s->n_grids; gi++) {
        const ycge_grid &g = s->grids[gi];
        GGrid &G = ggrids[gi];
        grid_record_init(g, G);
        const size_t cap = (size_t)G.nbx * G.nby * G.nbz * 512;
        const size_t off = (cells.size() + 255) & ~(size_t)255;
        if (off + cap >= ((size_t)1 << 32)) return c->fail(YCGE_ERR_UNSUPPORTED, "voxel storage exceeds 4 GiB");
        G.cell_offset = (uint32_t)off;
        cells.resize(off + cap, 0);
        G.lut_offset = (uint32_t)lut.size();
        int lo[3], hi[3];
        uint64_t brick_mask = 0;
        std::vector<std::pair<int32_t, int32_t>> seen;
        const int erc = encode_grid_host(c, g, gi, s->n_materials, G, cells.data() + off, lut, lo, hi, brick_mask, &seen);
        if (erc != YCGE_OK) return erc;
        grid_record_solid(G, lo, hi, brick_mask);
        A.codes.push_back(slot_codes_of(c, g, s->n_materials, &seen, lut.data() + G.lut_offset));          // (what a later edit of this grid codes its pairs by)
    }
    return YCGE_OK;
}

// what the object / scene-BVH step needs, kept for ycge_scene_update_objects, and the grid pool's view of the upload
int remember_for_updates(ycge_ctx *c, const ycge_scene *s, SceneArrays &A)
{
    c->gmeshes_host = A.gmeshes;
    c->n_materials = s->n_materials;
    c->max_mesh_depth = A.max_mesh_depth;
    c->materials_can_mirror = false;
    for (int i = 0; i < s->n_materials; i++) if (s->materials[i].reflectivity >= c->cfg.mirror_threshold) c->materials_can_mirror = true;
    c->grid_bounds.assign(s->n_grids, std::array<float, 6>{{0, 0, 0, -1, -1, -1}});
    for (int gi = 0; gi < s->n_grids; gi++) c->grid_bounds[gi] = grid_world_bounds(s->grids[gi]);
    c->grid_solid.resize(s->n_grids);
    for (int gi = 0; gi < s->n_grids; gi++)
    {
        for (int a = 0; a < 3; a++) { c->grid_solid[gi][a] = A.ggrids[gi].solid_lo[a]; c->grid_solid[gi][3 + a] = A.ggrids[gi].solid_hi[a]; }
        c->grid_solid[gi][6] = A.ggrids[gi].cull_t_limit;
    }
    A.has_grid = s->n_grids > 0;
    grid_pool_reset(c, A.ggrids, A.cells.size(), A.lut.size(), std::move(A.codes));          // (ycge_grid_encode.cpp: every grid of the upload is resident, nothing is free)
    mesh_pool_reset(c, A.tl_offset);                                                         // (ycge_mesh_pool.cpp: likewise every mesh)
    return YCGE_OK;
}

} // namespace ycge_host

extern "C" {

int ycge_validate_scene(const ycge_scene *scene, char *msg, size_t msg_bytes)
try {
    std::string m;
    const int rc = validate_scene(scene, m);
    if (msg && msg_bytes) { std::strncpy(msg, m.c_str(), msg_bytes - 1); msg[msg_bytes - 1] = 0; }
    return rc;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_scene_upload(ycge_ctx *c, const ycge_scene *s)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    std::string m;
    int rc = validate_scene(s, m);
    if (rc != YCGE_OK) return c->fail(rc, "%s", m.c_str());
    if ((rc = quiesce_all(c)) != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    c->have_scene = false;
    SceneArrays A;          // built once, by the steps in this order ...
    ObjectsHost oh;
    std::vector<ycge_prim> kept(s->prims, s->prims + s->n_prims);          // (what a later voxel edit installs again; made while a failure still leaves no scene)
    rc = flatten_materials(s, A);
    if (rc == YCGE_OK) rc = flatten_textures(s, A);
    if (rc == YCGE_OK) rc = build_mesh_arena(c, s, A);
    if (rc == YCGE_OK) rc = encode_grids(c, s, A);
    if (rc == YCGE_OK) rc = remember_for_updates(c, s, A);
    if (rc == YCGE_OK) rc = build_objects(c, s->prims, s->n_prims, oh);          // Scene.Objects + scene BVH
    if (rc != YCGE_OK) return rc;
    rc = on_root_then_peers(c, [&](ycge_ctx *x) {          // ... and installed on every device (a peer mirrors what check_scene_depth and flatten_objects read)
        x->max_mesh_depth = c->max_mesh_depth; x->n_materials = c->n_materials; x->materials_can_mirror = c->materials_can_mirror;
        return install_scene(x, A, oh, s);
    });
    (void)hipSetDevice(c->device);
    if (rc == YCGE_OK) c->grid_pool.owner.swap(oh.grid_owner);
    if (rc == YCGE_OK) c->last_prims.swap(kept);
    if (rc == YCGE_OK) rc = query_scene_changed(c);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_scene_update_lights(ycge_ctx *c, const ycge_light *lights, int32_t n_lights, const ycge_vec3 *ambient_color,
                             float ambient_intensity, const ycge_vec3 *top, const ycge_vec3 *bottom)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n_lights < 0 || (n_lights > 0 && !lights)) return c->fail(YCGE_ERR_INVALID_ARG, "bad light array");
    const int rc = on_root_then_peers(c, [&](ycge_ctx *x) {
        if (!x->have_scene) return x->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");          // (a peer whose install failed)
        int rc2 = quiesce(x);
        if (rc2 == YCGE_OK) rc2 = upload_lights(x, lights, n_lights);
        if (rc2 != YCGE_OK) return rc2;
        SceneDev &sd = x->sd;
        if (ambient_color) { sd.ambient[0] = ambient_color->x; sd.ambient[1] = ambient_color->y; sd.ambient[2] = ambient_color->z; sd.ambient_intensity = ambient_intensity; }
        if (top) { sd.bg_top[0] = top->x; sd.bg_top[1] = top->y; sd.bg_top[2] = top->z; }
        if (bottom) { sd.bg_bottom[0] = bottom->x; sd.bg_bottom[1] = bottom->y; sd.bg_bottom[2] = bottom->z; }
        return (int)YCGE_OK;
    });
    (void)hipSetDevice(c->device);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

// The next frame of a live texture (Renderer/Texture.cs:113-116: SampleBilinear reads IFrameReader.GetCurrentFramePtr())
int ycge_scene_update_texture(ycge_ctx *c, int32_t texture_index, const uint8_t *frame, size_t bytes)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (texture_index < 0 || (size_t)texture_index * 4 + 3 >= c->tex_info_host.size()) return c->fail(YCGE_ERR_INVALID_ARG, "texture index %d out of range", texture_index);
    const int32_t *info = c->tex_info_host.data() + (size_t)texture_index * 4;
    const int bpp = info[3] & 15;
    if (bpp == 0) return c->fail(YCGE_ERR_INVALID_ARG, "texture %d is static: upload the scene again to change it", texture_index);
    if (!frame || bytes != (size_t)info[1] * info[2] * bpp) return c->fail(YCGE_ERR_INVALID_ARG, "texture %d: a frame is %d x %d x %d bytes", texture_index, info[1], info[2], bpp);
    int rc = YCGE_OK;
    if (c->cfg.world_size == 1 && c->peers.empty() && (!c->last_stream || c->last_stream == c->stream)) {
        // Single device, no tiled call on a stream of the caller's: the traces of this context run on its own stream and - frames in flight of
        // the stage pipeline (render_frame_in_flight: odd frames from 4 096 tiles on) or of YCGE_PATH=m - on its second trace stream.  The
        // copy is queued on the first and ORDERED against the second both ways: it waits for what the second stream holds now (the trace that
        // still samples the old frame), and the second stream's next trace waits for it.  No device-wide wait, frames in flight stay in flight.
        // The caller's array is its own again when this returns: the frame is staged in page-locked memory first.
        HIP_TRY(c, hipSetDevice(c->device));
        if (c->stream2) {
            HIP_TRY(c, c->tex_order_ev.ensure());
            HIP_TRY(c, hipEventRecord(c->tex_order_ev, c->stream2));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->tex_order_ev, 0));
        }
        const int k = c->tex_stage_next; c->tex_stage_next ^= 1;
        if (c->tex_stage_busy[k]) { HIP_TRY(c, hipEventSynchronize(c->tex_stage_ev[k])); c->tex_stage_busy[k] = false; }      // (the copy of two updates ago)
        HIP_TRY(c, c->tex_stage[k].reserve(bytes));
        HIP_TRY(c, c->tex_stage_ev[k].ensure());
        std::memcpy(c->tex_stage[k].p, frame, bytes);
        HIP_TRY(c, hipMemcpyAsync(c->d_tex_pixels.p + info[0], c->tex_stage[k].p, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->tex_stage_ev[k], c->stream));
        if (c->stream2) HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->tex_stage_ev[k], 0));
        c->tex_stage_busy[k] = true;
        return YCGE_OK;
    }
    // several devices / a rank of a tiled frame / tiled calls on the caller's own streams: the scene changes while nothing runs
    rc = quiesce(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipMemcpy(c->d_tex_pixels.p + info[0], frame, bytes, hipMemcpyHostToDevice));
    for (ycge_ctx *p : c->peers) {
        if (hipSetDevice(p->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(p->d_tex_pixels.p + info[0], frame, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); rc = c->fail(YCGE_ERR_DEVICE, "texture frame copy failed on device %d", p->device); break; }
    }
    (void)hipSetDevice(c->device);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

// Scene.Update -> RebuildBVH when an entity moved (Scenes/Scene.cs:122-127, e.g. BobbingSphereEntity,
// TestScenesRandom.cs:708-714): new Scene.Objects records against the meshes, grids and materials of the last
// ycge_scene_upload.  Only the scene-level BVH is rebuilt (as in the reference: a Mesh keeps its own BVH).
int ycge_scene_update_objects(ycge_ctx *c, const ycge_prim *prims, int32_t n_prims)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n_prims < 0 || (n_prims > 0 && !prims)) return c->fail(YCGE_ERR_INVALID_ARG, "bad object array");
    std::vector<ycge_prim> kept(prims, prims + n_prims);          // (what a later voxel edit installs again)
    const int rc = ycge_host::update_objects(c, prims, n_prims);
    if (rc == YCGE_OK) c->last_prims.swap(kept);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

// Meshes and materials of a resident scene (the pool and the bodies: ycge_mesh_pool.cpp; the contract: include/ycge.h)
int ycge_scene_attach_meshes(ycge_ctx *c, const ycge_mesh *meshes, int32_t n, int32_t *out_mesh_index)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0 || (n > 0 && (!meshes || !out_mesh_index))) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_attach_meshes: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    return ycge_host::scene_attach_meshes(c, meshes, n, out_mesh_index);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_scene_detach_meshes(ycge_ctx *c, const int32_t *mesh_index, int32_t n)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0 || (n > 0 && !mesh_index)) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_meshes: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    return ycge_host::scene_detach_meshes(c, mesh_index, n);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_scene_append_materials(ycge_ctx *c, const ycge_material *materials, int32_t n, int32_t *out_first_index)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0 || (n > 0 && (!materials || !out_first_index))) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_append_materials: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    return ycge_host::scene_append_materials(c, materials, n, out_first_index);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_scene_attach_obj_mesh(ycge_ctx *c, int32_t auto_ground, int32_t normalize, float target_size, float scale, const float translate_or_target[3],
                               int32_t material, int32_t *out_mesh_index, float out_bounds[6])
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return ycge_host::obj_attach_mesh(c, auto_ground, normalize, target_size, scale, translate_or_target, material, out_mesh_index, out_bounds);
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"

// the body of ycge_scene_update_objects, also what ycge_scene_edit_voxels ends with when a held grid's record changed (with the kept list)
int ycge_host::update_objects(ycge_ctx *c, const ycge_prim *prims, int32_t n_prims)
{
    ObjectsHost oh;
    BoundsSoA items;
    int rc = flatten_objects(c, prims, n_prims, oh, items);       // host work first: the devices keep rendering the old objects meanwhile
    if (rc != YCGE_OK) return rc;
    // the tree itself is built on the device (ycge_bvh_build.hip) - on the host only for what that kernel does not take: no objects,
    // more than YCGE_BVH_DEV_MAX_ITEMS, or (reported by the kernel) a tree deeper than the reference's stack allows
    // ... and fewer objects than the measured crossover: one CU building a small tree loses to the host builder (300 objects: 168 us
    // against 105; config 5's 976: 559 against 354; 2 300: 687 against 1 533 - profiles/r02/f2_update_objects_timing.txt)
    bool on_device = !c->knobs.scene_bvh_host && n_prims >= 1 && n_prims >= c->knobs.scene_bvh_device_min && n_prims <= YCGE_BVH_DEV_MAX_ITEMS;
    if (!on_device) { rc = build_scene_tree_host(c, items, oh); if (rc != YCGE_OK) return rc; }
    rc = quiesce_all(c);
    if (rc != YCGE_OK) return rc;
    c->have_scene = false;
    // after an attach or a detach the kernel instantiation follows the grids Scene.Objects refer to, as after an upload of the equivalent
    // scene (which lists exactly those grids); a set the upload made keeps the upload's answer (its grid TABLE, used or not)
    if (c->grid_pool.streamed) c->has_grid = oh.any_grid_object;
    for (ycge_ctx *p : c->peers) p->has_grid = c->has_grid;
    const auto t0 = std::chrono::steady_clock::now();
    if (on_device) {
        rc = install_objects_device_built(c, c, oh, items);
        for (ycge_ctx *p : c->peers) {
            if (rc != YCGE_OK) break;
            rc = install_objects_device_built(p, c, oh, items);       // the same kernel on the same items: the same tree
            if (rc < 0) c->err = p->err;
        }
        if (rc == 1) {
            c->bvh_host_fallbacks++;
            on_device = false;
            rc = build_scene_tree_host(c, items, oh);
        } else if (rc == YCGE_OK) c->bvh_device_builds++;
    }
    if (!on_device && rc == YCGE_OK) rc = on_root_then_peers(c, [&](ycge_ctx *x) { return install_objects(x, oh); });
    c->bvh_last_build_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    (void)hipSetDevice(c->device);
    if (rc != YCGE_OK) return rc;
    mesh_pool_publish(c);          // (what streamed meshes and appended materials change in SceneDev follows here, with the objects that may use them: once they are installed)
    c->grid_pool.owner.swap(oh.grid_owner);
    c->have_scene = true;
    return query_scene_changed(c);
}

extern "C" {

// test / profiling hook: {device builds, host rebuilds after the kernel declined (a tree deeper than the reference's stack), host builds,
// microseconds of the last update's build + install, Array.Sort cases in the current tree (BVH.cs:389,419), depth of the current tree}
int ycge_debug_scene_bvh_stats(ycge_ctx *c, int64_t *out6)
try {
    if (!c || !out6) return YCGE_ERR_INVALID_ARG;
    out6[0] = c->bvh_device_builds; out6[1] = c->bvh_host_fallbacks; out6[2] = c->bvh_host_builds; out6[3] = (int64_t)c->bvh_last_build_us;
    out6[4] = c->scene_tree.sort_fallbacks; out6[5] = c->scene_tree.max_depth;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the scene nodes as the device holds them and SceneDev::walk_nodes (64 B each; the walk tree has 1 + 2 * YCGE_WALK_LEAF_NODES
// entries per scene node) + grid_owner; returns the scene node count (0: no walk tree), < 0 on an error
int ycge_debug_read_walk_tree(ycge_ctx *c, void *gnodes_out, void *walk_out, int32_t capacity_nodes, int32_t *grid_owner_out, int32_t n_grids, uint32_t *root_and_limit_out)
try {
    if (!c || !c->have_scene) return YCGE_ERR_INVALID_ARG;
    const int n = c->walk_scene_nodes;
    if (n == 0) return 0;
    if (!gnodes_out || !walk_out || capacity_nodes < n || !grid_owner_out || n_grids != (int)c->grid_solid.size() || !root_and_limit_out) return YCGE_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    { int rc2 = copy_out(c, gnodes_out, c->d_scene_nodes.p, (size_t)n * sizeof(GNode)); if (rc2 != YCGE_OK) return rc2;
      rc2 = copy_out(c, walk_out, c->d_walk_nodes.p, (size_t)n * (1 + 2 * YCGE_WALK_LEAF_NODES) * sizeof(GNode)); if (rc2 != YCGE_OK) return rc2;
      rc2 = copy_out(c, grid_owner_out, c->d_grid_owner.p, (size_t)n_grids * sizeof(int32_t)); if (rc2 != YCGE_OK) return rc2; }
    root_and_limit_out[0] = c->sd.walk_root_ref; std::memcpy(&root_and_limit_out[1], &c->sd.walk_t_limit, 4);
    return n;
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
