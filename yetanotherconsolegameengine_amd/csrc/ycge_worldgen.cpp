// ycge_worldgen.cpp - the host generator: WorldGenerator.GenerateChunkCells (Scenes/WorldGeneration/WorldGenerator.cs:95-203) on one
// thread, loop for loop, from the restatement in ycge_worldgen.h.  It is the yardstick the device generator (ycge_worldgen.hip) is held
// to, and what ycge_scene_generate_grids runs under YCGE_WORLDGEN_HOST.  ycge_worldgen_chunk_cells needs no context and no device.
// Below it, WorldManager.GenerateAndSaveWorld (WorldManager.cs:510-631) the same way: ycge_worldgen_world_cells.
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ycge.h"
#include "ycge_worldgen.h"
#include "ycge_worldgen_host.h"

struct ycge_ctx;
using namespace ycge;

namespace ycge_host {

int abi_catch(const ycge_ctx *c) noexcept;          // ycge_host.cpp: the exception barrier of the C-ABI (no context here: NULL)
int worldgen_check(const ycge_world *w, const char **why)
{
    if (!w) { *why = "null world"; return YCGE_ERR_INVALID_ARG; }
    if (w->chunk_size < 4 || w->chunk_size > 64) { *why = "chunk_size outside 4..64"; return YCGE_ERR_INVALID_ARG; }
    if (w->chunks_y < 1 || (int64_t)w->chunks_y * w->chunk_size > (1 << 20)) { *why = "chunks_y outside 1..2^20 / chunk_size"; return YCGE_ERR_INVALID_ARG; }
    return YCGE_OK;
}

// a chunk key both exports take: block coordinates within +-2^24, where they are exact in binary32 (the generator converts them) and
// key * chunk_size cannot overflow
int worldgen_key_check(const ycge_world *w, int32_t cx, int32_t cy, int32_t cz)
{
    const int32_t lim = (1 << 24) / w->chunk_size;
    const int32_t k[3] = {cx, cy, cz};
    for (int a = 0; a < 3; a++) if (k[a] < -lim || k[a] > lim) return YCGE_ERR_INVALID_ARG;
    return YCGE_OK;
}

// WorldGenerator.cs:104-154 with RiverNetwork.ComputeForChunk: the S x S records every cy of chunk column (cx, cz) shares
void worldgen_columns_host(const wg::World &W, int cx, int cz, wg::ColRec *cols)
{
    const int S = W.size, base_x = cx * S, base_z = cz * S;
    std::vector<int> tile((size_t)(S + 2) * (S + 2)), carved((size_t)S * S), river_water((size_t)S * S);
    std::vector<uint8_t> dir((size_t)S * S);
    for (int lx = -1; lx <= S; lx++)
        for (int lz = -1; lz <= S; lz++)
            tile[(size_t)(lx + 1) * (S + 2) + (lz + 1)] = wg::height_y(base_x + lx, base_z + lz, W);
    for (int lx = 0; lx < S; lx++)
        for (int lz = 0; lz < S; lz++)
            dir[(size_t)lx * S + lz] = (uint8_t)wg::d8_direction(tile.data(), S, lx, lz);
    for (int lx = 0; lx < S; lx++)
        for (int lz = 0; lz < S; lz++) {
            const size_t i = (size_t)lx * S + lz;
            carved[i] = wg::river_carve(wg::river_accum(dir.data(), S, lx, lz), wg::tile_at(tile.data(), S, lx, lz), W.sea, &river_water[i]);
        }
    for (int lx = 0; lx < S; lx++)
        for (int lz = 0; lz < S; lz++)
            cols[(size_t)lx * S + lz] = wg::column_record(carved.data(), S, lx, lz, base_x + lx, base_z + lz, river_water[(size_t)lx * S + lz], W);
}

// WorldGenerator.cs:156-202: the column fill, then FloraPlacer.PlaceTreesInChunk (FloraPlacer.cs:18-134)
void worldgen_fill_host(const wg::World &W, const wg::ColRec *cols, int cx, int cy, int cz, int32_t *cells, int32_t *any_solid_out)
{
    const int S = W.size, base_x = cx * S, base_y = cy * S, base_z = cz * S;
    bool any_solid = false;
    auto at = [&](int lx, int ly, int lz) { return cells + 2 * (((size_t)lx * S + ly) * S + lz); };
    for (int lx = 0; lx < S; lx++)
        for (int lz = 0; lz < S; lz++) {
            const wg::ColRec &R = cols[(size_t)lx * S + lz];
            for (int ly = 0; ly < S; ly++) {
                int mat, meta;
                wg::cell_at(R, base_y + ly, W, &mat, &meta);
                int32_t *c = at(lx, ly, lz);
                c[0] = mat; c[1] = meta;
                if (mat != 0) any_solid = true;
            }
        }
    for (int lx = 0; lx < S; lx++)
        for (int lz = 0; lz < S; lz++) {
            wg::Tree T;
            if (!wg::tree_at(cols[(size_t)lx * S + lz], lx, lz, base_x + lx, base_z + lz, base_y, W, &T)) continue;
            for (int t = 0; t < T.trunk_h; t++) {          // :72-81
                const int ly = T.trunk_base + t;
                if (ly < 0 || ly >= S) continue;
                int32_t *c = at(lx, ly, lz);
                if (wg::tree_may_replace(c[0])) { c[0] = wg::kWood; c[1] = 0; any_solid = true; }
            }
            bool any_leaves = false;          // :84-109
            for (int dy = wg::tree_dy_min(T); dy <= 2; dy++) {
                const int ly = T.canopy_base + dy;
                if (ly < 0 || ly >= S) continue;
                const int radius = wg::tree_radius(T, dy);
                for (int rx = -radius; rx <= radius; rx++) {
                    const int lx2 = lx + rx;
                    if (lx2 < 0 || lx2 >= S) continue;
                    for (int rz = -radius; rz <= radius; rz++) {
                        const int lz2 = lz + rz;
                        if (lz2 < 0 || lz2 >= S) continue;
                        int32_t *c = at(lx2, ly, lz2);
                        if (wg::tree_may_replace(c[0])) { c[0] = wg::kLeaves; c[1] = 0; any_solid = true; any_leaves = true; }
                    }
                }
            }
            if (!any_leaves) {          // :112-131
                const int ly = T.trunk_base + T.trunk_h - 1;
                if (ly >= 0 && ly < S)
                    for (int rx = -1; rx <= 1; rx++) {
                        const int lx2 = lx + rx;
                        if (lx2 < 0 || lx2 >= S) continue;
                        for (int rz = -1; rz <= 1; rz++) {
                            const int lz2 = lz + rz;
                            if (lz2 < 0 || lz2 >= S) continue;
                            int32_t *c = at(lx2, ly, lz2);
                            if (c[0] == wg::kAir) { c[0] = wg::kLeaves; c[1] = 0; any_solid = true; }
                        }
                    }
            }
        }
    *any_solid_out = any_solid ? 1 : 0;
}


// ---------------------------------------------------------------------------------------------------------------- GenerateAndSaveWorld
int worldgen_window_check(const ycge_world *w, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, const char **why)
{
    if (chunks_x < 1 || chunks_z < 1) { *why = "chunks_x or chunks_z < 1"; return YCGE_ERR_INVALID_ARG; }
    const int64_t S = w->chunk_size, lim = 1 << 24;
    const int64_t nx = chunks_x * S, nz = chunks_z * S, ny = (int64_t)w->chunks_y * S;
    if (origin_bx < -lim || origin_bz < -lim || origin_bx + nx - 1 > lim || origin_bz + nz - 1 > lim) { *why = "the window leaves +-2^24 blocks"; return YCGE_ERR_INVALID_ARG; }
    if (nx * ny >= ((int64_t)1 << 30) || nx * ny * nz >= ((int64_t)1 << 30)) { *why = "nx * ny * nz >= 2^30"; return YCGE_ERR_INVALID_ARG; }          // (nx, nz <= 2^25 + 1, ny <= 2^20)
    return YCGE_OK;
}

// WorldManager.cs:521-560 and the feature descriptors, loop for loop
void world_fields_host(const wg::World &W, const wg::Window &N, WorldFields &F)
{
    const int nx = N.nx, nz = N.nz;
    const size_t n = (size_t)nx * nz;
    F.ground0.resize(n); F.ground.resize(n); F.river_water.resize(n); F.dir.resize(n); F.accum.resize(n); F.rec.resize(n); F.feat.resize(n);
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) F.ground0[(size_t)x * nz + z] = wg::height_y(N.ox + x, N.oz + z, W);
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) F.dir[(size_t)x * nz + z] = (uint8_t)wg::d8_global(F.ground0.data(), nx, nz, x, z);
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) {
            const size_t i = (size_t)x * nz + z;
            F.accum[i] = wg::river_accum_global(F.dir.data(), nx, nz, x, z);
            F.ground[i] = wg::river_carve(F.accum[i], F.ground0[i], W.sea, &F.river_water[i]);
        }
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) {
            const size_t i = (size_t)x * nz + z;
            F.rec[i] = wg::column_record_global(F.ground.data(), N, x, z, F.river_water[i], W);
            F.feat[i] = wg::feature_at(F.rec[i], N.ox + x, N.oz + z, W);
        }
}

// WorldManager.cs:562-606: the voxel fill, then FloraPlacer.PlaceTreesGlobal (FloraPlacer.cs:137-254) as the serial loops it is, from the
// feature descriptors.  cells: the VG01 payload, (x * ny + y) * nz + z.
void world_serial_host(const wg::World &W, const wg::Window &N, const wg::ColRec *rec, const uint32_t *feat, int32_t *cells)
{
    const int nx = N.nx, nz = N.nz, ny = W.height;
    auto at = [&](int x, int y, int z) { return cells + 2 * (((size_t)x * ny + y) * nz + z); };
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) {
            const wg::ColRec &R = rec[(size_t)x * nz + z];
            for (int y = 0; y < ny; y++) { int32_t *c = at(x, y, z); int mat, meta; wg::cell_at_global(R, y, W, &mat, &meta); c[0] = mat; c[1] = meta; }
        }
    for (int gx = 0; gx < nx; gx++) {
        for (int gz = 0; gz < nz; gz++) {
            const uint32_t d = feat[(size_t)gx * nz + gz];
            if (wg::feat_kind(d) != wg::kFeatTree) continue;
            const wg::Tree T = wg::feat_tree(d, rec[(size_t)gx * nz + gz].ground);
            for (int t = 0; t < T.trunk_h; t++) {          // :171-176
                const int y = T.trunk_base + t;
                if (y < 0 || y >= ny) break;
                int32_t *c = at(gx, y, gz);
                if (wg::tree_may_replace(c[0])) { c[0] = wg::kWood; c[1] = 0; }
            }
            bool any_leaves = false;          // :179-195
            for (int dy = wg::tree_dy_min(T); dy <= 2; dy++) {
                const int y = T.canopy_base + dy;
                if (y < 0 || y >= ny) continue;
                const int radius = wg::tree_radius(T, dy);
                for (int rx = -radius; rx <= radius; rx++) {
                    const int x2 = gx + rx;
                    if (x2 < 0 || x2 >= nx) continue;
                    for (int rz = -radius; rz <= radius; rz++) {
                        const int z2 = gz + rz;
                        if (z2 < 0 || z2 >= nz) continue;
                        int32_t *c = at(x2, y, z2);
                        if (wg::tree_may_replace(c[0])) { c[0] = wg::kLeaves; c[1] = 0; any_leaves = true; }
                    }
                }
            }
            if (!any_leaves) {          // :196-211
                const int y = T.trunk_base + T.trunk_h - 1;
                if (y >= 0 && y < ny)
                    for (int rx = -1; rx <= 1; rx++) {
                        const int x2 = gx + rx;
                        if (x2 < 0 || x2 >= nx) continue;
                        for (int rz = -1; rz <= 1; rz++) {
                            const int z2 = gz + rz;
                            if (z2 < 0 || z2 >= nz) continue;
                            int32_t *c = at(x2, y, z2);
                            if (c[0] == wg::kAir) { c[0] = wg::kLeaves; c[1] = 0; }
                        }
                    }
            }
        }
        for (int gz = 0; gz < nz; gz++) {          // :214-252, after the trees of this x
            const uint32_t d = feat[(size_t)gx * nz + gz];
            const int gY = rec[(size_t)gx * nz + gz].ground;
            if (wg::feat_kind(d) == wg::kFeatCactus) {
                const int height = wg::feat_cactus_h(d);
                for (int t = 1; t <= height; t++) {
                    const int y = gY + t;
                    if (y >= ny) break;
                    int32_t *c = at(gx, y, gz);
                    if (c[0] == wg::kAir) { c[0] = wg::kWood; c[1] = 0; }
                }
            } else if (wg::feat_kind(d) == wg::kFeatRock) {
                const int y = gY + 1;
                if (y >= ny) continue;
                for (int rx = -1; rx <= 1; rx++) {
                    const int x2 = gx + rx;
                    if (x2 < 0 || x2 >= nx) continue;
                    for (int rz = -1; rz <= 1; rz++) {
                        const int z2 = gz + rz;
                        if (z2 < 0 || z2 >= nz) continue;
                        if ((rx < 0 ? -rx : rx) + (rz < 0 ? -rz : rz) > 1) continue;
                        int32_t *c = at(x2, y, z2);
                        if (c[0] == wg::kAir) { c[0] = wg::kStone; c[1] = 1; }
                    }
                }
            }
        }
    }
}

// The same cells the way the kernels make them (ycge_worldpregen.hip), on the host: the fallback flags to their fixed point, then every
// cell by wg::world_cell.  Returns the number of passes over the trees (the last one changes nothing).
int world_gather_host(const wg::World &W, const wg::Window &N, const wg::ColRec *rec, const uint32_t *feat, int32_t *cells)
{
    const int nx = N.nx, nz = N.nz, ny = W.height;
    std::vector<uint8_t> fallback((size_t)nx * nz, 0);
    int passes = 0;
    for (bool changed = true; changed;) {
        changed = false;
        passes++;
        std::vector<uint8_t> next = fallback;
        for (int x = 0; x < nx; x++)
            for (int z = 0; z < nz; z++) {
                const size_t i = (size_t)x * nz + z;
                if (wg::feat_kind(feat[i]) != wg::kFeatTree) continue;
                const uint8_t f = wg::tree_any_leaves(rec, feat, fallback.data(), N, W, x, z) ? 0 : 1;
                if (f != fallback[i]) { next[i] = f; changed = true; }
            }
        fallback.swap(next);
    }
    for (int x = 0; x < nx; x++)
        for (int y = 0; y < ny; y++)
            for (int z = 0; z < nz; z++) {
                int mat, meta;
                wg::world_cell(rec, feat, fallback.data(), N, W, x, y, z, &mat, &meta);
                int32_t *c = cells + 2 * (((size_t)x * ny + y) * nz + z);
                c[0] = mat; c[1] = meta;
            }
    return passes;
}

int world_cells_host(const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t *cells_out)
{
    const wg::World W = wg::make_world(world->chunk_size, world->chunks_y, world->world_seed);
    const wg::Window N = {chunks_x * W.size, chunks_z * W.size, origin_bx, origin_bz};
    WorldFields F;
    world_fields_host(W, N, F);
    world_serial_host(W, N, F.rec.data(), F.feat.data(), cells_out);
    return YCGE_OK;
}

}  // namespace ycge_host

extern "C" {
int ycge_worldgen_chunk_cells(const ycge_world *world, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t *any_solid_out)
try {
    const char *why = nullptr;
    const int rc = ycge_host::worldgen_check(world, &why);
    if (rc != YCGE_OK) return rc;
    if (!cells_out || !any_solid_out) return YCGE_ERR_INVALID_ARG;
    if (ycge_host::worldgen_key_check(world, cx, cy, cz) != YCGE_OK) return YCGE_ERR_INVALID_ARG;
    const wg::World W = wg::make_world(world->chunk_size, world->chunks_y, world->world_seed);
    std::vector<wg::ColRec> cols((size_t)W.size * W.size);
    ycge_host::worldgen_columns_host(W, cx, cz, cols.data());
    ycge_host::worldgen_fill_host(W, cols.data(), cx, cy, cz, cells_out, any_solid_out);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ---- test hooks (include/ycge_hooks.h): the restatement's pieces on a caller's inputs, host only
// GenMath: hash_out[i] = FastHash(ix[i], 0, iz[i], seed); noise_out[i] = GradientNoise2D(x[i], z[i], seed)
int ycge_host_worldgen_noise(int32_t n, const int32_t *ix, const int32_t *iz, const float *x, const float *z, int32_t seed, uint32_t *hash_out, float *noise_out)
try {
    if (n < 0 || (n > 0 && (!ix || !iz || !x || !z || !hash_out || !noise_out))) return YCGE_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) { hash_out[i] = wg::fast_hash(ix[i], 0, iz[i], seed); noise_out[i] = wg::gradient_noise2(x[i], z[i], seed); }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
// TerrainNoise.HeightY at n points
int ycge_host_worldgen_height(const ycge_world *world, int32_t n, const int32_t *gx, const int32_t *gz, int32_t *height_out)
try {
    const char *why = nullptr;
    if (ycge_host::worldgen_check(world, &why) != YCGE_OK || n < 0 || (n > 0 && (!gx || !gz || !height_out))) return YCGE_ERR_INVALID_ARG;
    const wg::World W = wg::make_world(world->chunk_size, world->chunks_y, world->world_seed);
    for (int i = 0; i < n; i++) height_out[i] = wg::height_y(gx[i], gz[i], W);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
// RiverNetwork.ComputeForChunk on a caller's (size + 2)^2 height tile (index (lx + 1) * (size + 2) + (lz + 1)):
// per chunk cell (index lx * size + lz) the D8 code, accum, carved ground, river surface
int ycge_host_worldgen_river(const int32_t *tile, int32_t size, int32_t sea, int32_t *dir_out, float *accum_out, int32_t *carved_out, int32_t *river_water_out)
try {
    if (!tile || size < 1 || size > 64 || !dir_out || !accum_out || !carved_out || !river_water_out) return YCGE_ERR_INVALID_ARG;
    std::vector<uint8_t> dir((size_t)size * size);
    for (int lx = 0; lx < size; lx++)
        for (int lz = 0; lz < size; lz++) dir_out[lx * size + lz] = dir[(size_t)lx * size + lz] = (uint8_t)wg::d8_direction(tile, size, lx, lz);
    for (int lx = 0; lx < size; lx++)
        for (int lz = 0; lz < size; lz++) {
            const int i = lx * size + lz;
            accum_out[i] = wg::river_accum(dir.data(), size, lx, lz);
            carved_out[i] = wg::river_carve(accum_out[i], wg::tile_at(tile, size, lx, lz), sea, &river_water_out[i]);
        }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
// river_carve alone at a given accumulation (the formulas behind the threshold, which no chunk reaches)
int ycge_host_worldgen_carve(float accum, int32_t ground, int32_t sea, int32_t *carved_out, int32_t *river_water_out)
try {
    if (!carved_out || !river_water_out) return YCGE_ERR_INVALID_ARG;
    *carved_out = wg::river_carve(accum, ground, sea, river_water_out);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ---- GenerateAndSaveWorld
int ycge_worldgen_world_cells(const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t *cells_out)
try {
    const char *why = nullptr;
    int rc = ycge_host::worldgen_check(world, &why);
    if (rc == YCGE_OK) rc = ycge_host::worldgen_window_check(world, chunks_x, chunks_z, origin_bx, origin_bz, &why);
    if (rc != YCGE_OK) return rc;
    if (!cells_out) return YCGE_ERR_INVALID_ARG;
    return ycge_host::world_cells_host(world, chunks_x, chunks_z, origin_bx, origin_bz, cells_out);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: the 2-D fields of a window from the host code, each nx * nz in x * nz + z order (NULL: skipped).  climate: BiomeMap's
// dryness verdict alone (Forest or Desert, whatever the height); rock: StrataMap's noise verdict.
int ycge_host_worldgen_world_fields(const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t *ground0_out,
                                               int32_t *ground_out, int32_t *dir_out, float *accum_out, float *slope_out, int32_t *biome_out, int32_t *water_out,
                                               uint32_t *feature_out, int32_t *climate_out, int32_t *rock_out)
try {
    const char *why = nullptr;
    int rc = ycge_host::worldgen_check(world, &why);
    if (rc == YCGE_OK) rc = ycge_host::worldgen_window_check(world, chunks_x, chunks_z, origin_bx, origin_bz, &why);
    if (rc != YCGE_OK) return rc;
    const wg::World W = wg::make_world(world->chunk_size, world->chunks_y, world->world_seed);
    const wg::Window N = {chunks_x * W.size, chunks_z * W.size, origin_bx, origin_bz};
    ycge_host::WorldFields F;
    ycge_host::world_fields_host(W, N, F);
    const size_t n = (size_t)N.nx * N.nz;
    for (size_t i = 0; i < n; i++) {
        if (ground0_out) ground0_out[i] = F.ground0[i];
        if (ground_out) ground_out[i] = F.ground[i];
        if (dir_out) dir_out[i] = F.dir[i];
        if (accum_out) accum_out[i] = F.accum[i];
        if (slope_out) slope_out[i] = F.rec[i].slope;
        if (biome_out) biome_out[i] = F.rec[i].biome_rock & 0xff;
        if (water_out) water_out[i] = F.rec[i].water;
        if (feature_out) feature_out[i] = F.feat[i];
        if (climate_out) climate_out[i] = wg::biome_evaluate(N.ox + (int)(i / N.nz), N.oz + (int)(i % N.nz), W.sea + wg::kBeachBuffer + 1, W.sea, W);
        if (rock_out) rock_out[i] = F.rec[i].biome_rock >> 8;
    }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: RiverNetworkGlobal.Compute (and WorldManager.cs:536) on a caller's nx * nz heights: D8 code, accum, carved ground, river surface
int ycge_host_worldgen_river_global(const int32_t *ground, int32_t nx, int32_t nz, int32_t sea, int32_t *dir_out, float *accum_out, int32_t *carved_out,
                                               int32_t *river_water_out)
try {
    if (!ground || nx < 1 || nz < 1 || (int64_t)nx * nz > (1 << 24) || !dir_out || !accum_out || !carved_out || !river_water_out) return YCGE_ERR_INVALID_ARG;
    std::vector<uint8_t> dir((size_t)nx * nz);
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) dir_out[x * nz + z] = dir[(size_t)x * nz + z] = (uint8_t)wg::d8_global(ground, nx, nz, x, z);
    for (int x = 0; x < nx; x++)
        for (int z = 0; z < nz; z++) {
            const int i = x * nz + z;
            accum_out[i] = wg::river_accum_global(dir.data(), nx, nz, x, z);
            carved_out[i] = wg::river_carve(accum_out[i], ground[i], sea, &river_water_out[i]);
        }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: the voxel fill and the flora pass on CALLER-GIVEN fields of nx x nz columns (any sizes >= 1; ground in 0..height-1; biome a
// Biome value; rock 0..2; feature a descriptor of ycge_worldgen.h, or NULL: wg::feature_at of the given fields with origin (0, 0)) - gather == 0: the serial loops of ycge_worldgen_world_cells, != 0: the
// kernels' scheme on the host (fallback flags to a fixed point, then wg::world_cell per cell).  passes_out: 0, or the gather's passes.
int ycge_host_worldgen_world_from_fields(const ycge_world *world, int32_t nx, int32_t nz, const int32_t *ground, const int32_t *water, const float *slope,
                                                    const int32_t *biome, const int32_t *rock, const uint32_t *feature, int32_t gather, int32_t *cells_out,
                                                    int32_t *passes_out)
try {
    const char *why = nullptr;
    if (ycge_host::worldgen_check(world, &why) != YCGE_OK || nx < 1 || nz < 1 || !ground || !water || !slope || !biome || !rock || !cells_out || !passes_out)
        return YCGE_ERR_INVALID_ARG;
    const wg::World W = wg::make_world(world->chunk_size, world->chunks_y, world->world_seed);
    if ((int64_t)nx * nz * W.height >= ((int64_t)1 << 30)) return YCGE_ERR_INVALID_ARG;
    const wg::Window N = {nx, nz, 0, 0};
    std::vector<wg::ColRec> rec((size_t)nx * nz);
    for (size_t i = 0; i < rec.size(); i++) {
        if (ground[i] < 0 || ground[i] >= W.height) return YCGE_ERR_INVALID_ARG;
        rec[i].ground = ground[i]; rec[i].water = water[i]; rec[i].slope = slope[i]; rec[i].biome_rock = (biome[i] & 0xff) | ((rock[i] & 3) << 8);
    }
    std::vector<uint32_t> feat(rec.size());
    for (size_t i = 0; i < rec.size(); i++) feat[i] = feature ? feature[i] : wg::feature_at(rec[i], (int)(i / (size_t)nz), (int)(i % (size_t)nz), W);
    *passes_out = 0;
    if (gather) *passes_out = ycge_host::world_gather_host(W, N, rec.data(), feat.data(), cells_out);
    else ycge_host::world_serial_host(W, N, rec.data(), feat.data(), cells_out);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
} // extern "C"
