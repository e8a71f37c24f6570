// ycge_worldgen_host.h - what ycge_worldgen.cpp (host generator) and ycge_worldgen.hip / ycge_worldpregen.hip (device generators) offer
// ycge_scene_generate_grids and ycge_scene_generate_world (ycge_worldgen_scene.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "ycge_worldgen.h"

struct ycge_world;

namespace ycge {
// one chunk of a fill launch: its key, its chunk column's slot among the launch's column records, where its 2 * S^3 int32 go
struct WgChunk {
    int32_t cx, cy, cz, col;
    int32_t *cells;
};
static_assert(sizeof(WgChunk) == 24, "WgChunk must be 24 B");
// the 2-D fields of a pregen window on one device, each nx * nz in x * nz + z order (ycge_worldpregen.hip)
struct WpFields {
    int32_t *ground0, *ground, *river_water;          // HeightY; after the river pass; the river surface
    uint8_t *dir, *fallback;                          // D8 code; 1: the column's tree takes its fallback crown
    wg::ColRec *rec;
    uint32_t *feat;                                   // feature descriptor (ycge_worldgen.h)
    int32_t *reach;                                   // the highest y a feature rooted within kFeatReach columns may write (-1: none near)
    uint32_t *changed;                                // one word: flags the last k_wp_any_leaves pass flipped
    uint32_t *occupied;                               // one word per chunk, ((cx * chunks_y) + cy) * chunks_z + cz: != 0 when a cell of the finished chunk is not Air
};
}  // namespace ycge

namespace ycge_host {
int worldgen_check(const ycge_world *w, const char **why);
int worldgen_key_check(const ycge_world *w, int32_t cx, int32_t cy, int32_t cz);          // (after worldgen_check)
void worldgen_columns_host(const ycge::wg::World &W, int cx, int cz, ycge::wg::ColRec *cols /* S * S */);
void worldgen_fill_host(const ycge::wg::World &W, const ycge::wg::ColRec *cols, int cx, int cy, int cz, int32_t *cells /* 2 * S^3 */, int32_t *any_solid_out);
// GenerateAndSaveWorld
struct WorldFields {
    std::vector<int32_t> ground0, ground, river_water;
    std::vector<uint8_t> dir;
    std::vector<float> accum;
    std::vector<ycge::wg::ColRec> rec;
    std::vector<uint32_t> feat;
};
int worldgen_window_check(const ycge_world *w, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, const char **why);          // (after worldgen_check)
void world_fields_host(const ycge::wg::World &W, const ycge::wg::Window &N, WorldFields &F);
void world_serial_host(const ycge::wg::World &W, const ycge::wg::Window &N, const ycge::wg::ColRec *rec, const uint32_t *feat, int32_t *cells);
int world_gather_host(const ycge::wg::World &W, const ycge::wg::Window &N, const ycge::wg::ColRec *rec, const uint32_t *feat, int32_t *cells);
int world_cells_host(const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t *cells_out);          // (checked by the caller)
}  // namespace ycge_host

extern "C" {
// k_wg_columns: col_keys = n_cols x {cx, cz}; cols = n_cols x S*S records; col_top[k] = max over the column's cells of max(ground, water)
int ycge_launch_worldgen_columns(const int32_t *col_keys, int n_cols, const ycge::wg::World *W, ycge::wg::ColRec *cols, int32_t *col_top, void *stream);
// k_wg_fill, then k_wg_trees: the chunks' raw cells, any_solid[k] (zeroed by the caller) per chunk
int ycge_launch_worldgen_fill(const ycge::WgChunk *chunks, int n_chunks, const ycge::wg::World *W, const ycge::wg::ColRec *cols, uint32_t *any_solid, void *stream);
// ycge_worldpregen.hip.  The 2-D stages of a window up to the feature descriptors, the reach and zeroed fallback flags (k_wp_height, k_wp_d8,
// k_wp_carve, k_wp_columns, k_wp_reach) ...
int ycge_launch_worldpregen_fields(const ycge::wg::World *W, const ycge::wg::Window *N, const ycge::WpFields *F, void *stream);
// ... one pass of the anyLeaves fixed point: every tree's flag from the flags as they are into `next` (nx * nz bytes), *F->changed = how many flipped ...
int ycge_launch_worldpregen_any_leaves(const ycge::wg::World *W, const ycge::wg::Window *N, const ycge::WpFields *F, uint8_t *next, void *stream);
// ... which chunks of the finished world hold anything (k_wp_occupied; F->occupied is zeroed here) ...
int ycge_launch_worldpregen_occupied(const ycge::wg::World *W, const ycge::wg::Window *N, const ycge::WpFields *F, int chunks_y, int chunks_z, size_t n_chunks, void *stream);
// ... and the cells of chunks (cx, cy, cz = chunk coordinates in the window; col is not read), any_solid[k] (zeroed by the caller) per chunk
int ycge_launch_worldpregen_fill(const ycge::WgChunk *chunks, int n_chunks, const ycge::wg::World *W, const ycge::wg::Window *N, const ycge::WpFields *F, uint32_t *any_solid,
                                 void *stream);
// ... or the x-planes [x0, x0 + planes) of the finished world in VG01 order (k_wp_planes) to `cells`, 2 * planes * ny * nz int32: plane x0's first cell
int ycge_launch_worldpregen_planes(const ycge::wg::World *W, const ycge::wg::Window *N, const ycge::WpFields *F, int32_t x0, int32_t planes, int32_t *cells, void *stream);
}
