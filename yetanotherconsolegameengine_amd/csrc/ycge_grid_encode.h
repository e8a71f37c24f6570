// ycge_grid_encode.h - what ycge_grid_encode.cpp hands k_grid_encode (ycge_grid_encode.hip): one descriptor per grid of a batch and the
// record each grid's workgroups reduce into.
#pragma once
#include <stdint.h>

namespace ycge {

#define YCGE_ENC_RUN 4                  // bricks along z a workgroup of k_grid_encode takes (a 32^3 chunk: one workgroup per brick column)
#define YCGE_ENC_LUT_ENTRIES 256        // LUT region of an attached grid: code 0 = empty, 1 + k = lookup entry k, n_lookup + 1 = default_material
#define YCGE_ENC_MAX_LOOKUP 254         // larger lookup tables take the host encoder

struct GridEncDesc {
    const int32_t *cells;               // the raw (matId, metaId) pairs on the device, ycge_grid.cells order
    uint8_t *out;                       // nbx * nby * nbz bricks of 512 bytes
    int32_t *lut;                       // YCGE_ENC_LUT_ENTRIES entries
    const int32_t *lookup;              // n_lookup x {matId, metaId, material}
    int32_t nx, ny, nz;
    int32_t nbx, nby, nbz;
    int32_t n_lookup;
    int32_t default_material;           // < 0: a lookup miss is an error
    uint32_t first_wg;                  // this grid's workgroups are [first_wg, next grid's first_wg)
    uint32_t maskable;                  // at most 64 bricks: the brick mask is kept
    uint32_t pad[2];
};
static_assert(sizeof(GridEncDesc) == 80, "GridEncDesc must be 80 B");

struct GridEncResult {                  // set by the host to {nx, ny, nz}, {-1, -1, -1}, 0, 0, 0xffffffff, 0
    int32_t lo[3], hi[3];               // index box of the solid voxels
    uint32_t mask_lo, mask_hi;          // bit b: brick b holds a solid voxel
    uint32_t bad_cell;                  // the lowest cell (ycge_grid.cells order) with no material: a lookup miss with default_material < 0
    uint32_t any_miss;                  // some solid cell missed the lookup table
    uint32_t pad[2];
};
static_assert(sizeof(GridEncResult) == 48, "GridEncResult must be 48 B");

}  // namespace ycge
