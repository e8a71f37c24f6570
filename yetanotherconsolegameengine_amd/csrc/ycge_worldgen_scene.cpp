// ycge_worldgen_scene.cpp - chunks generated into a resident scene: ycge_scene_generate_grids (WorldGenerator.GenerateChunkCells per chunk key) and
// ycge_scene_generate_world (WorldManager.GenerateAndSaveWorld for a window).  Each export finds out which chunks hold anything and hands those to
// attach_grids_from (ycge_grid_encode.cpp) with a CellSource whose groups are the sub-batches of the fill kernels: the cells are made on every device, where
// k_grid_encode reads them, or by ycge_worldgen.cpp (YCGE_WORLDGEN_HOST; a lookup table k_grid_encode does not take).  All before the attach changes scratch buffers only.
#include <algorithm>
#include <map>

#include "ycge_worldgen_cells.h"

namespace ycge_host {
namespace {

// ycge_scene_generate_grids: EVERY key of the call (the Air chunks' cells are made too when the caller wants them); grid k of the attach is chunk grid_key[k]
struct ChunkCells : GeneratedCells {
    std::vector<int> grid_key;
    std::vector<wg::ColRec> host_cols;               // YCGE_WORLDGEN_HOST: n_cols x S * S
    int32_t *cells_out;                              // the caller's, per key; or NULL
    ChunkCells(const ycge_world *world, bool device, int32_t *out) : GeneratedCells("ycge_scene_generate_grids", "k_wg_fill", world, device), cells_out(out) {}
    int32_t *out_of(int i) const { return cells_out + (size_t)i * (chunk_bytes() / 4); }
    int launch(ycge_ctx *x, const WgChunk *chunks, int m, uint32_t *any_solid) override { return ycge_launch_worldgen_fill(chunks, m, &W, (const wg::ColRec *)x->d_wg_cols.p, any_solid, x->stream); }
    // the host generator: from the call's column records, or (a lookup table too large for k_grid_encode, whoever makes the other chunks) the chunk's own.  Holds something?
    bool host_chunk(int i, int32_t *cells) const
    {
        const size_t S2 = (size_t)W.size * W.size;
        std::vector<wg::ColRec> own;
        if (host_cols.empty()) { own.resize(S2); worldgen_columns_host(W, keys[(size_t)i][0], keys[(size_t)i][2], own.data()); }
        int32_t any_solid = 0;
        worldgen_fill_host(W, own.empty() ? host_cols.data() + (size_t)col[(size_t)i] * S2 : own.data(), keys[(size_t)i][0], keys[(size_t)i][1], keys[(size_t)i][2], cells, &any_solid);
        return any_solid != 0;
    }
    int write(ycge_ctx *root, size_t k, const ycge_grid &, int32_t *cells) override
    {
        if (!host_chunk(grid_key[k], cells)) return wrong(root, grid_key[k], true);
        if (cells_out) std::memcpy(out_of(grid_key[k]), cells, chunk_bytes());
        return YCGE_OK;
    }
    // chunks ks filled and, on the root, their cells to the caller if asked
    int fill_and_take(ycge_ctx *root, ycge_ctx *x, const std::vector<int> &ks, uint8_t *d_head, const std::vector<int32_t *> &d_cells, bool solid)
    {
        int rc = fill_chunks(root, x, ks, d_head, d_cells, solid);
        for (size_t j = 0; j < ks.size() && rc == YCGE_OK && x == root && cells_out; j++) rc = copy_out(root, out_of(ks[j]), d_cells[j], chunk_bytes());
        return rc;
    }
    int fill(ycge_ctx *root, ycge_ctx *x, const std::vector<int> &group, uint8_t *d_head, const std::vector<int32_t *> &d_cells) override
    {
        std::vector<int> ks;
        for (int k : group) ks.push_back(grid_key[(size_t)k]);
        return fill_and_take(root, x, ks, d_head, d_cells, true);
    }
};

// What both exports begin with, in this order: the refusals - the context, the world, `own` (the export's other arguments), the scene, the grid g0 every
// chunk's record starts from, the n keys - then the frames in flight joined, on the root's device.  n == 0: the call asks for no chunk, and proto is not looked at.
template <class Own> int generate_begin(ycge_ctx *c, const char *fn, const ycge_world *world, const ycge_grid *proto, const int32_t *keys, int32_t n, Own own, ycge_grid &g0)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    const char *why = nullptr;
    if (worldgen_check(world, &why) != YCGE_OK) return c->fail(YCGE_ERR_INVALID_ARG, "%s: %s", fn, why);
    const int rc = own();
    if (rc != YCGE_OK) return rc;
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    static const int32_t no_cells[2] = {0, 0};          // (validate_grid wants a pointer; a generated grid's cells are never read through it)
    g0 = *proto;
    g0.nx = g0.ny = g0.nz = world->chunk_size; g0.voxel_size = world->voxel_size; g0.cells = no_cells;
    std::string m;
    const int vrc = validate_grid(g0, 0, c->n_materials, m);
    if (vrc != YCGE_OK) return c->fail(vrc, "%s", m.c_str());
    for (int k = 0; keys && k < n; k++)
        if (worldgen_key_check(world, keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]) != YCGE_OK)          // (block coordinates stay exact in binary32, as the generator assumes)
            return c->fail(YCGE_ERR_INVALID_ARG, "%s: key %d is outside +-2^24 blocks", fn, k);
    const int qrc = quiesce_all(c);
    if (qrc != YCGE_OK) return qrc;
    HIP_TRY(c, hipSetDevice(c->device));
    return YCGE_OK;
}

// the grid of chunk (cx, cy, cz): WorldManager.cs:722-726, 761-768
ycge_grid chunk_grid(const ycge_grid &g0, const ycge_world *world, int cx, int cy, int cz)
{
    const int S = world->chunk_size;
    ycge_grid g = g0;
    g.min_corner.x = world->world_min.x + (float)(cx * S) * world->voxel_size.x;
    g.min_corner.y = world->world_min.y + (float)(cy * S) * world->voxel_size.y;
    g.min_corner.z = world->world_min.z + (float)(cz * S) * world->voxel_size.z;
    return g;
}

// the chunks that hold something attached (grid j is chunk which[j] of the call's n); every chunk's index to the caller, -1 for one that holds nothing
int attach_chunks(ycge_ctx *c, const std::vector<ycge_grid> &grids, CellSource &src, const std::vector<int> &which, size_t n, int32_t *out_grid_index)
{
    std::vector<int32_t> idx(grids.size(), -1);
    const int rc = grids.empty() ? YCGE_OK : attach_grids_from(c, grids.data(), (int32_t)grids.size(), idx.data(), src);
    if (rc != YCGE_OK) return rc;
    std::fill(out_grid_index, out_grid_index + n, -1);
    for (size_t j = 0; j < which.size(); j++) out_grid_index[which[j]] = idx[j];
    return YCGE_OK;
}

}  // namespace

int wp_make_fields(ycge_ctx *c, const char *fn, bool is_root, uint8_t *base, const wg::World &W, const wg::Window &N, int chunks_y, int chunks_z, hipStream_t stream,
                   const WpReadBack &read_back, int &passes, double us[3], uint32_t *occupied)
{
    const size_t n_cols = (size_t)N.nx * N.nz, n_chunks = (size_t)(N.nx / W.size) * chunks_y * (size_t)chunks_z;
    WpFields F;
    wp_layout(base, n_cols, n_chunks, &F);
    uint8_t *flags[2] = {F.fallback, wp_next_flags(F, n_cols)};
    auto t0 = std::chrono::steady_clock::now();
    int e = ycge_launch_worldpregen_fields(&W, &N, &F, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_* launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(stream));
    if (is_root) us[0] = us_since(t0);
    t0 = std::chrono::steady_clock::now();
    int done = 0, cur = 0;
    for (;;) {          // anyLeaves: from flags[cur] into flags[1 - cur] until a pass flips nothing (then both hold the fixed point)
        F.fallback = flags[cur];
        e = ycge_launch_worldpregen_any_leaves(&W, &N, &F, flags[1 - cur], stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_any_leaves launch failed: %s", hipGetErrorString((hipError_t)e));
        done++;
        if (!is_root) { if (done == passes) break; cur = 1 - cur; continue; }
        HIP_TRY(c, hipStreamSynchronize(stream));
        uint32_t changed = 0;
        const int rc = read_back(&changed, F.changed, sizeof changed);
        if (rc != YCGE_OK) return rc;
        if (!changed) break;
        if ((size_t)done > n_cols + 1) return c->fail(YCGE_ERR_INTERNAL, "%s: the anyLeaves passes do not settle", fn);
        cur = 1 - cur;
    }
    F.fallback = flags[0];          // (the last pass flipped nothing: both buffers hold the fixed point, and wp_layout names this one)
    if (!is_root) { HIP_TRY(c, hipStreamSynchronize(stream)); return YCGE_OK; }
    passes = done; us[1] = us_since(t0);
    t0 = std::chrono::steady_clock::now();
    e = ycge_launch_worldpregen_occupied(&W, &N, &F, chunks_y, chunks_z, n_chunks, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_occupied launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(stream));
    const int rc = read_back(occupied, F.occupied, n_chunks * 4);
    if (rc != YCGE_OK) return rc;
    us[2] = us_since(t0);
    return YCGE_OK;
}

}  // namespace ycge_host

extern "C" {

// ycge_scene_generate_grids: the chunk columns first (every 2-D field of WorldGenerator.GenerateChunkCells, once per distinct (cx, cz)) - their tops say which chunks hold anything, and only those take part in the attach
int ycge_scene_generate_grids(ycge_ctx *c, const ycge_world *world, const int32_t *keys, int32_t n, const ycge_grid *proto, int32_t *out_grid_index, int32_t *cells_out)
try {
    ycge_grid g0;
    int rc = generate_begin(c, "ycge_scene_generate_grids", world, proto, keys, n, [&] {
        return n < 0 || (n > 0 && (!keys || !out_grid_index)) || !proto ? c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_grids: bad array (n = %d)", n) : YCGE_OK;
    }, g0);
    if (rc != YCGE_OK || n == 0) return rc;
    const DeviceGuard guard(c->device);

    ChunkCells src(world, !c->knobs.worldgen_host, cells_out);
    const int S = world->chunk_size;
    const size_t S2 = (size_t)S * S;
    std::vector<std::array<int32_t, 2>> col_keys;
    std::map<std::pair<int32_t, int32_t>, int32_t> seen;
    for (int k = 0; k < n; k++) {
        const auto ins = seen.insert({{keys[3 * k], keys[3 * k + 2]}, (int32_t)col_keys.size()});
        if (ins.second) col_keys.push_back({{keys[3 * k], keys[3 * k + 2]}});
        src.keys.push_back({{keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]}});
        src.col.push_back(ins.first->second);
    }
    const size_t n_cols = col_keys.size();
    std::vector<int32_t> col_top(n_cols);
    c->worldgen_last_us[0] = c->worldgen_last_us[1] = 0;
    const size_t cols_bytes = align_up(n_cols * S2 * sizeof(wg::ColRec), 256), keys_bytes = align_up(n_cols * 8, 256);
    if (!src.on_device) {
        src.host_cols.resize(n_cols * S2);
        for (size_t j = 0; j < n_cols; j++) {
            worldgen_columns_host(src.W, col_keys[j][0], col_keys[j][1], src.host_cols.data() + j * S2);
            int32_t top = INT32_MIN;
            for (size_t i = 0; i < S2; i++) { const wg::ColRec &R = src.host_cols[j * S2 + i]; top = std::max(top, std::max(R.ground, R.water)); }
            col_top[j] = top;
        }
    } else {
        for (ycge_ctx *x : contexts_of(c)) {
            HIP_TRY(c, hipSetDevice(x->device));
            const size_t need = cols_bytes + keys_bytes + n_cols * 4;
            if (x->d_wg_cols.cap < need) HIP_TRY(c, x->d_wg_cols.alloc(need));
            uint8_t *d_keys = x->d_wg_cols.p + cols_bytes, *d_top = d_keys + keys_bytes;
            const auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(c, hipMemcpyAsync(d_keys, col_keys.data(), n_cols * 8, hipMemcpyHostToDevice, x->stream));
            const int e = ycge_launch_worldgen_columns((const int32_t *)d_keys, (int)n_cols, &src.W, (wg::ColRec *)x->d_wg_cols.p, (int32_t *)d_top, x->stream);
            if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wg_columns launch failed: %s", hipGetErrorString((hipError_t)e));
            HIP_TRY(c, hipStreamSynchronize(x->stream));
            if (x == c) {
                c->worldgen_last_us[0] = us_since(t0);
                rc = copy_out(c, col_top.data(), d_top, n_cols * 4);
                if (rc != YCGE_OK) return rc;
            }
        }
        HIP_TRY(c, hipSetDevice(c->device));
    }
    // a chunk holds something exactly when a column reaches into or above it: Water up to localWater, ground below (trees stand on ground of their own chunk)
    std::vector<int> air_k;
    std::vector<ycge_grid> grids;
    for (int k = 0; k < n; k++) {
        if (col_top[(size_t)src.col[(size_t)k]] < src.keys[(size_t)k][1] * S) { air_k.push_back(k); continue; }
        src.grid_key.push_back(k);
        grids.push_back(chunk_grid(g0, world, src.keys[(size_t)k][0], src.keys[(size_t)k][1], src.keys[(size_t)k][2]));
    }
    // the empty chunks' cells, when asked for: made like the others (and found empty), in launches of their own
    if (cells_out && !src.on_device) {
        for (int k : air_k)
            if (src.host_chunk(k, src.out_of(k))) return src.wrong(c, k, false);
    } else if (cells_out) {
        const size_t slot = align_up(src.chunk_bytes(), 256);
        const size_t per = std::max<size_t>(1, std::min<size_t>(kGenGroupMax, std::min<size_t>((size_t)64 << 20, c->knobs.enc_group_bytes) / slot));
        for (size_t first = 0; first < air_k.size(); first += per) {
            const std::vector<int> ks(air_k.begin() + first, air_k.begin() + std::min(first + per, air_k.size()));
            const size_t head = src.head_bytes(ks.size());
            if (c->d_enc_in.cap < head + ks.size() * slot) HIP_TRY(c, c->d_enc_in.alloc(head + ks.size() * slot));
            std::vector<int32_t *> d_cells(ks.size());
            for (size_t j = 0; j < ks.size(); j++) d_cells[j] = (int32_t *)(c->d_enc_in.p + head + j * slot);
            rc = src.fill_and_take(c, c, ks, c->d_enc_in.p, d_cells, false);
            if (rc != YCGE_OK) return rc;
        }
    }
    rc = attach_chunks(c, grids, src, src.grid_key, (size_t)n, out_grid_index);
    c->worldgen_last_us[1] = src.fill_us;
    if (rc != YCGE_OK) return rc;
    // who made the cells: the kernels, or the host generator (the knob; a lookup table too large for k_grid_encode).  An empty chunk's cells are made only when cells_out asks.
    const bool solid_on_host = !src.on_device || proto->n_lookup > YCGE_ENC_MAX_LOOKUP;
    const int64_t n_solid = (int64_t)grids.size(), n_air = cells_out ? (int64_t)air_k.size() : 0;
    c->worldgen_host_chunks += (solid_on_host ? n_solid : 0) + (src.on_device ? 0 : n_air);
    c->worldgen_device_chunks += (solid_on_host ? 0 : n_solid) + (src.on_device ? n_air : 0);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// ycge_scene_generate_world: the 2-D fields of the window first (on every device), the anyLeaves flags to their fixed point, then one
// word per chunk - does it hold anything (AttachChunkFromPreloaded, WorldManager.cs:704-720: any cell not Air, trees from other chunks
// included; EXACT, chunk by chunk: between a column's ground and a neighbour's canopy above it a whole small chunk can be Air) - and the
// attach of the chunks that do.
int ycge_scene_generate_world(ycge_ctx *c, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, const ycge_grid *proto,
                              int32_t *out_grid_index, int32_t *cells_out)
try {
    ycge_grid g0;
    int rc = generate_begin(c, "ycge_scene_generate_world", world, proto, nullptr, 1, [&] {
        const char *why = nullptr;
        if (worldgen_window_check(world, chunks_x, chunks_z, origin_bx, origin_bz, &why) != YCGE_OK) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_world: %s", why);
        return !out_grid_index || !proto ? c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_world: null argument") : YCGE_OK;
    }, g0);
    if (rc != YCGE_OK) return rc;
    const DeviceGuard guard(c->device);

    const int S = world->chunk_size, chunks_y = world->chunks_y;
    // (a table k_grid_encode does not take: every chunk is encoded on the host, from the host's cells)
    WindowCells src(world, !c->knobs.worldgen_host && proto->n_lookup <= YCGE_ENC_MAX_LOOKUP, wg::Window{chunks_x * S, chunks_z * S, origin_bx, origin_bz});
    const wg::World &W = src.W; const wg::Window &N = src.N;
    const size_t n_cols = (size_t)N.nx * N.nz, ny = (size_t)W.height, n_chunks = (size_t)chunks_x * chunks_y * chunks_z;
    const size_t world_i32 = 2 * n_cols * ny;
    std::vector<uint32_t> occupied(n_chunks, 0);          // per chunk, (cx, cy, cz) with cx outermost: != 0 when it holds anything
    std::vector<int32_t> host_world;
    for (double &u : c->worldpregen_last_us) u = 0;
    c->worldpregen_last_passes = 0;
    if (!src.on_device) {
        int32_t *w = cells_out;
        if (!w) { host_world.resize(world_i32); w = host_world.data(); }
        world_cells_host(world, chunks_x, chunks_z, origin_bx, origin_bz, w);
        src.host_world = w;
        for (size_t x = 0; x < (size_t)N.nx; x++)
            for (size_t y = 0; y < ny; y++) {
                const int32_t *row = w + 2 * ((x * ny + y) * N.nz);
                for (size_t z = 0; z < (size_t)N.nz; z++)
                    if (row[2 * z] != 0) occupied[((x / S) * chunks_y + y / S) * chunks_z + z / S] = 1;
            }
    } else {
        int root_passes = 0;
        for (ycge_ctx *x : contexts_of(c)) {          // (the root first: a peer repeats its passes without reading anything back)
            HIP_TRY(c, hipSetDevice(x->device));
            const size_t need = wp_layout(nullptr, n_cols, n_chunks, nullptr);
            if (x->d_wg_cols.cap < need) HIP_TRY(c, x->d_wg_cols.alloc(need));
            rc = wp_make_fields(c, "ycge_scene_generate_world", x == c, x->d_wg_cols.p, W, N, chunks_y, chunks_z, x->stream,
                                [&](void *dst, const void *from, size_t bytes) { return copy_out(c, dst, from, bytes); }, root_passes, c->worldpregen_last_us, occupied.data());
            if (rc != YCGE_OK) return rc;
        }
        c->worldpregen_last_passes = root_passes;
        HIP_TRY(c, hipSetDevice(c->device));
        if (cells_out) { std::memset(cells_out, 0, world_i32 * 4); src.world_out = cells_out; }          // (a chunk that holds nothing is (Air, 0) throughout)
    }
    std::vector<ycge_grid> grids;
    std::vector<int> solid_k;
    for (int cx = 0; cx < chunks_x; cx++)
        for (int cy = 0; cy < chunks_y; cy++)
            for (int cz = 0; cz < chunks_z; cz++) {
                const size_t k = ((size_t)cx * chunks_y + cy) * chunks_z + cz;
                if (!occupied[k]) continue;
                grids.push_back(chunk_grid(g0, world, cx, cy, cz));
                src.keys.push_back({{cx, cy, cz}}); src.col.push_back(0);
                solid_k.push_back((int)k);
            }
    rc = attach_chunks(c, grids, src, solid_k, n_chunks, out_grid_index);
    c->worldpregen_last_us[3] = src.fill_us;
    if (rc != YCGE_OK) return rc;
    (src.on_device ? c->worldgen_device_chunks : c->worldgen_host_chunks) += (int64_t)n_chunks;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: the last ycge_scene_generate_world on the root device - {anyLeaves passes (the last flips nothing), us of the
// 2-D field kernels, of the anyLeaves pass loop (WALL time: each pass is a launch, a stream synchronise and a 4-byte read-back), of the
// occupancy kernel and its read-back, of the fill kernels}
int ycge_debug_worldpregen_stats(ycge_ctx *c, int64_t *out5)
try {
    if (!c || !out5) return YCGE_ERR_INVALID_ARG;
    out5[0] = c->worldpregen_last_passes;
    for (int a = 0; a < 4; a++) out5[1 + a] = (int64_t)c->worldpregen_last_us[a];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: {chunks made on the device, chunks made on the host, the last ycge_scene_generate_grids' column kernel and fill + tree kernels in microseconds (root device)}
int ycge_debug_worldgen_stats(ycge_ctx *c, int64_t *out4)
try {
    if (!c || !out4) return YCGE_ERR_INVALID_ARG;
    out4[0] = c->worldgen_device_chunks; out4[1] = c->worldgen_host_chunks; out4[2] = (int64_t)c->worldgen_last_us[0]; out4[3] = (int64_t)c->worldgen_last_us[1];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
