// ycge_worldgen.cpp - the host generator: WorldGenerator.GenerateChunkCells (Scenes/WorldGeneration/WorldGenerator.cs:95-203) on one
// thread, loop for loop, from the restatement in ycge_worldgen.h.  It is the yardstick the device generator (ycge_worldgen.hip) is held
// to, and what ycge_scene_generate_grids runs under YCGE_WORLDGEN_HOST.  ycge_worldgen_chunk_cells needs no context and no device.
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ycge.h"
#include "ycge_worldgen.h"
#include "ycge_worldgen_host.h"

using namespace ycge;

namespace ycge_host {

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

}  // namespace ycge_host

extern "C" int ycge_worldgen_chunk_cells(const ycge_world *world, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t *any_solid_out)
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
catch (const std::bad_alloc &) { return YCGE_ERR_OUT_OF_MEMORY; }
catch (...) { return YCGE_ERR_INTERNAL; }

// ---- test hooks (include/ycge_hooks.h): the restatement's pieces on a caller's inputs, host only
// GenMath: hash_out[i] = FastHash(ix[i], 0, iz[i], seed); noise_out[i] = GradientNoise2D(x[i], z[i], seed)
extern "C" int ycge_host_worldgen_noise(int32_t n, const int32_t *ix, const int32_t *iz, const float *x, const float *z, int32_t seed, uint32_t *hash_out, float *noise_out)
try {
    if (n < 0 || (n > 0 && (!ix || !iz || !x || !z || !hash_out || !noise_out))) return YCGE_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) { hash_out[i] = wg::fast_hash(ix[i], 0, iz[i], seed); noise_out[i] = wg::gradient_noise2(x[i], z[i], seed); }
    return YCGE_OK;
}
catch (...) { return YCGE_ERR_INTERNAL; }
// TerrainNoise.HeightY at n points
extern "C" int ycge_host_worldgen_height(const ycge_world *world, int32_t n, const int32_t *gx, const int32_t *gz, int32_t *height_out)
try {
    const char *why = nullptr;
    if (ycge_host::worldgen_check(world, &why) != YCGE_OK || n < 0 || (n > 0 && (!gx || !gz || !height_out))) return YCGE_ERR_INVALID_ARG;
    const wg::World W = wg::make_world(world->chunk_size, world->chunks_y, world->world_seed);
    for (int i = 0; i < n; i++) height_out[i] = wg::height_y(gx[i], gz[i], W);
    return YCGE_OK;
}
catch (...) { return YCGE_ERR_INTERNAL; }
// RiverNetwork.ComputeForChunk on a caller's (size + 2)^2 height tile (index (lx + 1) * (size + 2) + (lz + 1)):
// per chunk cell (index lx * size + lz) the D8 code, accum, carved ground, river surface
extern "C" int ycge_host_worldgen_river(const int32_t *tile, int32_t size, int32_t sea, int32_t *dir_out, float *accum_out, int32_t *carved_out, int32_t *river_water_out)
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
catch (...) { return YCGE_ERR_INTERNAL; }
// river_carve alone at a given accumulation (the formulas behind the threshold, which no chunk reaches)
extern "C" int ycge_host_worldgen_carve(float accum, int32_t ground, int32_t sea, int32_t *carved_out, int32_t *river_water_out)
try {
    if (!carved_out || !river_water_out) return YCGE_ERR_INVALID_ARG;
    *carved_out = wg::river_carve(accum, ground, sea, river_water_out);
    return YCGE_OK;
}
catch (...) { return YCGE_ERR_INTERNAL; }
