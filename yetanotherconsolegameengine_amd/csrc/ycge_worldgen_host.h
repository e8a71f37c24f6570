// ycge_worldgen_host.h - what ycge_worldgen.cpp (host generator) and ycge_worldgen.hip (device generator) offer ycge_scene_generate_grids
// (ycge_grid_encode.cpp).
#pragma once
#include <stdint.h>

#include "ycge_worldgen.h"

struct ycge_world;

namespace ycge {
// one chunk of a fill launch: its key, its chunk column's slot among the launch's column records, where its 2 * S^3 int32 go
struct WgChunk {
    int32_t cx, cy, cz, col;
    int32_t *cells;
};
static_assert(sizeof(WgChunk) == 24, "WgChunk must be 24 B");
}  // namespace ycge

namespace ycge_host {
int worldgen_check(const ycge_world *w, const char **why);
int worldgen_key_check(const ycge_world *w, int32_t cx, int32_t cy, int32_t cz);          // (after worldgen_check)
void worldgen_columns_host(const ycge::wg::World &W, int cx, int cz, ycge::wg::ColRec *cols /* S * S */);
void worldgen_fill_host(const ycge::wg::World &W, const ycge::wg::ColRec *cols, int cx, int cy, int cz, int32_t *cells /* 2 * S^3 */, int32_t *any_solid_out);
}  // namespace ycge_host

extern "C" {
// k_wg_columns: col_keys = n_cols x {cx, cz}; cols = n_cols x S*S records; col_top[k] = max over the column's cells of max(ground, water)
int ycge_launch_worldgen_columns(const int32_t *col_keys, int n_cols, const ycge::wg::World *W, ycge::wg::ColRec *cols, int32_t *col_top, void *stream);
// k_wg_fill, then k_wg_trees: the chunks' raw cells, any_solid[k] (zeroed by the caller) per chunk
int ycge_launch_worldgen_fill(const ycge::WgChunk *chunks, int n_chunks, const ycge::wg::World *W, const ycge::wg::ColRec *cols, uint32_t *any_solid, void *stream);
}
