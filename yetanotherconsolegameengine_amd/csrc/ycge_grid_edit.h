// ycge_grid_edit.h - what ycge_grid_edit.cpp hands the kernels of ycge_grid_edit.hip: the ops of a ycge_scene_edit_voxels call with their
// pairs turned into code bytes, one work record per touched brick, one descriptor per edited grid for the solid-box reduction.
#pragma once
#include <stdint.h>

#include "ycge_grid_encode.h"

namespace ycge {

#define YCGE_EDIT_MAX_RECORDS (1u << 26)   // bricks one call may touch (one workgroup each)

struct GridEditOp {                     // one op, in its grid's index space; the ops of a grid lie together, in list order
    int32_t lo[3], hi[3];               // inclusive, inside the grid
    uint32_t code;                      // the byte every cell of the box becomes
    uint32_t pad;
};
static_assert(sizeof(GridEditOp) == 32, "GridEditOp must be 32 B");

struct GridEditRecord {                 // one touched brick: a workgroup of k_grid_edit
    uint64_t brick;                     // byte offset of its 512 bytes in the cell arena
    int32_t bx, by, bz;                 // its brick coordinates: cell (x, y, z) of it is voxel (8 bx + x, 8 by + y, 8 bz + z)
    uint32_t op_first, op_count;        // its grid's ops
    uint32_t pad;
};
static_assert(sizeof(GridEditRecord) == 32, "GridEditRecord must be 32 B");

struct GridSolidDesc {                  // one edited grid: its workgroups of k_grid_solid take two bricks each
    uint64_t cells;                     // byte offset of its first brick in the cell arena
    int32_t nbx, nby, n_bricks;
    uint32_t first_wg;                  // this grid's workgroups are [first_wg, next grid's first_wg)
    uint32_t maskable;                  // at most 64 bricks: the brick mask is kept
    uint32_t pad;
};
static_assert(sizeof(GridSolidDesc) == 32, "GridSolidDesc must be 32 B");

// k_grid_solid reduces into a GridEncResult (ycge_grid_encode.h), set by the host as for k_grid_encode; bad_cell and any_miss stay as set.

}  // namespace ycge
