// ycge_world_store.h - what ycge_world_store.cpp hands the kernels of ycge_world_store.hip: the shape of a resident VG01 world and one
// launch record per chunk of a slice.
#pragma once
#include <stdint.h>

namespace ycge {

#define YCGE_WORLD_STORE_SLAB_BYTES_DEFAULT ((size_t)64 << 20)   // staged per slab of a load: two such page-locked buffers are held while it runs (crossover not yet measured)
#define YCGE_WORLD_STORE_MAX_CHUNK 1024
#define YCGE_WORLD_STORE_MAX_CHUNKS (1 << 24)

struct WsShape {                        // the world (cells in VG01 order: x, then y, then z fastest) and its chunks
    int32_t nx, ny, nz, S;
    int32_t ncx, ncy, ncz, pad;         // chunks per axis: ceil(n / S); the last one of an axis is clipped
};

struct WsChunk {
    uint64_t src;                       // the chunk's first cell in the store, in cells: ((cx * S) * ny + cy * S) * nz + cz * S
    int32_t sx, sy, sz;                 // its clipped sizes
    int32_t pad;
    int32_t *dst;                       // sx * sy * sz cells in ycge_grid.cells order
};
static_assert(sizeof(WsChunk) == 32, "WsChunk must be 32 B");

#define YCGE_WS_EDIT_OPS_PER_LAUNCH 32768   // ops of one k_ws_edit launch (its gridDim.y)

struct WsEditOp {                       // one op of ycge_world_store_edit: every cell of the inclusive box, in store cell coordinates, becomes {mat, meta}
    int32_t lo[3], hi[3];
    int32_t mat, meta;
};
static_assert(sizeof(WsEditOp) == 32, "WsEditOp must be 32 B");

// ---- the pool of materialised chunks beside a fields store (ycge_world_store_reserve_edits): slot s is the S^3 cells at
// pool + s * stride bytes, ycge_grid.cells order - what k_wp_fill writes
#define YCGE_WS_POOL_BATCH_DEFAULT 32768    // records of one pool launch (its gridDim.y); YCGE_WS_POOL_BATCH at ycge_create

struct WsPoolEdit {                     // one op of ycge_world_store_edit clipped against one chunk it touches
    int32_t slot;
    int32_t lo[3], hi[3];               // the inclusive box inside the chunk, 0..S-1
    int32_t mat, meta, pad;
};
static_assert(sizeof(WsPoolEdit) == 40, "WsPoolEdit must be 40 B");

struct WsPoolCopy {                     // a whole slot into the cells of a grid of an attach
    int32_t slot, pad;
    int32_t *dst;
};
static_assert(sizeof(WsPoolCopy) == 16, "WsPoolCopy must be 16 B");

struct WsPoolPlanes {                   // the part of a slot that lies in a slab of x-planes: planes lx0 .. lx0 + n - 1 of chunk (., cy, cz), the first of them plane `px` of the slab
    int32_t slot, lx0, n, px, cy, cz, pad[2];
};
static_assert(sizeof(WsPoolPlanes) == 32, "WsPoolPlanes must be 32 B");

}  // namespace ycge

extern "C" {
// k_ws_edit: the m ops at `ops` (device memory, list order; m <= YCGE_WS_EDIT_OPS_PER_LAUNCH) into the store at `cells`, the later op winning where boxes overlap;
// max_cells: the largest box among them
int ycge_launch_world_store_edit(int32_t *cells, const ycge::WsShape *shape, const ycge::WsEditOp *ops, int m, uint64_t max_cells, void *stream);
// k_ws_occupied over the x-planes [x0, x0 + planes) of the store at `cells` (the whole store's base): occupied[(cx * ncy + cy) * ncz + cz] |= 1 for
// every chunk with a cell of mat != 0 in those planes.  The words are the caller's to zero, once, before the first slab.
int ycge_launch_world_store_occupied(const int32_t *cells, const ycge::WsShape *shape, int32_t x0, int32_t planes, uint32_t *occupied, void *stream);
// k_ws_slice: chunk k of the m records at `chunks` (device memory) from the store at `cells` into its dst; max_cells: the largest sx * sy * sz among them
int ycge_launch_world_store_slice(const int32_t *cells, const ycge::WsShape *shape, const ycge::WsChunk *chunks, int m, size_t max_cells, void *stream);
// The pool's kernels.  pool, stride (bytes a slot, a multiple of 16), S: the pool of this device; records in device memory, m of them, m <= 65535.
// k_ws_pool_edit: the records sorted by slot, list order inside a slot, the later record of a slot winning where boxes overlap; max_cells: the largest box
int ycge_launch_world_store_pool_edit(uint8_t *pool, size_t stride, int S, const ycge::WsPoolEdit *recs, int m, uint64_t max_cells, void *stream);
// k_ws_pool_occupied: words[j] |= 1 when slot slots[j] holds a cell of mat != 0.  The words are the caller's to zero.
int ycge_launch_world_store_pool_occupied(const uint8_t *pool, size_t stride, int S, const int32_t *slots, int m, uint32_t *words, void *stream);
// k_ws_pool_copy: slot recs[j].slot into recs[j].dst (S^3 cells, 16-byte aligned, room for an even number of cells), 16 bytes a lane
int ycge_launch_world_store_pool_copy(const uint8_t *pool, size_t stride, int S, const ycge::WsPoolCopy *recs, int m, void *stream);
// k_ws_pool_planes: the records' parts of their slots into a slab of x-planes of ny x nz cells in VG01 order (slab: plane 0 of it)
int ycge_launch_world_store_pool_planes(const uint8_t *pool, size_t stride, int S, const ycge::WsPoolPlanes *recs, int m, int32_t *slab, int32_t ny, int32_t nz, void *stream);
}
