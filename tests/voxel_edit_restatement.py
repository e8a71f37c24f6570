"""A numpy restatement of voxel edits (ycge_scene_edit_voxels / ycge_world_store_edit) and the drawn grids and op lists the GPU tests use.
Nothing here touches the library: tests/test_voxel_edit_cpu.py checks on these inputs alone that every condition the GPU tests rely on is
present, so no GPU test can pass by being vacuous.

An op is a row of nine ints, a ycge_voxel_edit: {grid_index, lo xyz, hi xyz, mat_id, meta_id}; the box is inclusive."""
import numpy as np

# the lookup table every drawn grid is attached with: entry k -> material k; a solid pair it lacks falls to DEFAULT_MATERIAL
PALETTE = [(1, 0), (1, 1), (2, 0), (3, 0), (4, 2), (5, 1)]
DEFAULT_MATERIAL = 9
N_MATERIALS = 12
MISS_PAIR = (40, 3)            # a solid pair the table lacks
AIR_PAIR = (-3, 2)             # air: mat_id < 0 with a non-zero meta


def op(lo, hi, pair, grid=0):
    return [int(grid), *(int(v) for v in lo), *(int(v) for v in hi), int(pair[0]), int(pair[1])]


def apply_ops(cells, ops):
    """cells int32 [nx, ny, nz, 2] with the boxes of `ops` written in list order (the later op wins); a new array."""
    out = np.array(cells, np.int32, copy=True)
    for o in np.asarray(ops, np.int64).reshape(-1, 9):
        out[o[1]:o[4] + 1, o[2]:o[5] + 1, o[3]:o[6] + 1] = (o[7], o[8])
    return out


def materials_of(cells):
    """what ycge_debug_read_grid reports for these cells under PALETTE / DEFAULT_MATERIAL: the material per cell, -1 for air"""
    out = np.full(cells.shape[:3], -1, np.int32)
    solid = cells[..., 0] > 0
    out[solid] = DEFAULT_MATERIAL
    for k, (a, b) in enumerate(PALETTE):
        out[solid & (cells[..., 0] == a) & (cells[..., 1] == b)] = k
    return out


def code_identity(cells, host_encoded):
    """An int64 per cell that is equal for two cells exactly when a slot gives them the same code byte: air is one code whatever its
    ids; a device-encoded slot codes by its lookup table (all misses share default_material's code), a host-encoded slot by the pair."""
    solid = cells[..., 0] > 0
    if host_encoded:
        ident = (cells[..., 0].astype(np.int64) << 32) | (cells[..., 1].astype(np.int64) & 0xffffffff)
    else:
        ident = materials_of(cells).astype(np.int64) + 1
        ident[solid & (ident == DEFAULT_MATERIAL + 1)] = 1000          # the miss code (no PALETTE entry maps to DEFAULT_MATERIAL)
    return np.where(solid, ident, 0)


def solid_box(cells):
    """(lo xyz, hi xyz) of the cells with mat_id > 0, or None"""
    idx = np.argwhere(cells[..., 0] > 0)
    return None if idx.size == 0 else (tuple(idx.min(0)), tuple(idx.max(0)))


def brick_mask(cells):
    """the set of 8^3 bricks (bx, by, bz) that hold a solid cell; None for a grid of more than 64 bricks (no mask is kept)"""
    nb = [(n + 7) // 8 for n in cells.shape[:3]]
    if nb[0] * nb[1] * nb[2] > 64:
        return None
    return {tuple(v) for v in np.argwhere(cells[..., 0] > 0) // 8}


def record_changed(before, after):
    return solid_box(before) != solid_box(after) or brick_mask(before) != brick_mask(after)


def expected_info(before, after, host_encoded):
    """(cells whose code changed, bricks that hold one, 1 if the record changed) of one grid"""
    changed = code_identity(before, host_encoded) != code_identity(after, host_encoded)
    bricks = {tuple(v) for v in np.argwhere(changed) // 8}
    return int(changed.sum()), len(bricks), int(record_changed(before, after))


# ------------------------------------------------------------------------------------------------ the encoder case
def drawn_grids():
    """label -> (cells, min corner, voxel size): the grids of the encoder test"""
    from yetanotherconsolegameengine_amd import scenes
    rng = np.random.default_rng(23)

    def cells(shape, fill):
        c = np.zeros(shape + (2,), np.int32)
        solid = rng.random(shape) < fill
        pick = rng.integers(0, len(PALETTE), shape)
        pal = np.asarray(PALETTE, np.int32)
        c[..., 0] = np.where(solid, pal[pick, 0], rng.integers(-2, 1, shape))
        c[..., 1] = np.where(solid, pal[pick, 1], rng.integers(0, 3, shape))
        return c

    one = np.zeros((16, 16, 16, 2), np.int32); one[15, 15, 15] = PALETTE[2]
    world = np.ascontiguousarray(scenes.make_voxel_world(96, 128, 96)[32:64, 32:64, 32:64])
    return {
        "13 x 9 x 21": (cells((13, 9, 21), 0.5), (1.5, -2.0, 3.25), (0.5, 0.75, 1.25)),
        "1 x 1 x 1": (np.array([[[PALETTE[3]]]], np.int32), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
        "9 x 8 x 7 all air": (np.zeros((9, 8, 7, 2), np.int32), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
        "16^3 one voxel": (one, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
        "40 x 33 x 47": (cells((40, 33, 47), 0.2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
        "a chunk of the world": (world, (-16.0, 32.0, -16.0), (1.0, 1.0, 1.0)),
    }


def drawn_calls(label, cells):
    """The op lists of one grid, one ycge_scene_edit_voxels call each: mixed boxes; a slab that shrinks the solid box; the whole grid to air;
    one first solid cell."""
    rng = np.random.default_rng(sum(map(ord, label)))
    dims = np.asarray(cells.shape[:3])

    def box(max_side=5):
        lo = rng.integers(0, dims)
        return lo, np.minimum(dims - 1, lo + rng.integers(0, max_side, 3))

    first = []
    axis = int(np.argmax(dims))
    if dims[axis] > 8:                                   # a box across a brick border
        lo, hi = box(3)
        lo[axis], hi[axis] = 6, min(int(dims[axis]) - 1, 9)
        first.append(op(lo, hi, PALETTE[0]))
    lo, hi = box()
    first.append(op(lo, hi, PALETTE[1]))                 # two boxes that share a cell, different pairs: the order matters
    first.append(op(lo, np.minimum(dims - 1, hi + 1), PALETTE[2]))
    first.append(op(*box(), AIR_PAIR))
    first.append(op(*box(3), MISS_PAIR))                 # falls to default_material
    calls = [first]
    now = apply_ops(cells, first)
    sb = solid_box(now)
    if sb is not None and any(h > l for l, h in zip(*sb)):          # the far plane of the solid box on its longest axis goes: the box shrinks
        a = int(np.argmax(np.asarray(sb[1]) - np.asarray(sb[0])))
        lo, hi = np.zeros(3, np.int64), dims - 1
        lo[a] = hi[a] = sb[1][a]
        calls.append([op(lo, hi, (0, 0))])
    calls.append([op((0, 0, 0), dims - 1, (-1, 5))])     # empties the grid
    calls.append([op(p := rng.integers(0, dims), p, PALETTE[3])])          # the first solid cell of an all-air grid
    return calls


# ------------------------------------------------------------------------------------------------ the world-store case
STORE_DIMS, STORE_CHUNK = (40, 24, 40), 16


def store_world():
    """40 x 24 x 40 with chunks of 16: the far chunks of every axis are clipped (8 cells); chunk (2, 1, 2) is empty, chunk (1, 0, 1) is not"""
    rng = np.random.default_rng(31)
    w = np.zeros(STORE_DIMS + (2,), np.int32)
    w[..., 0] = np.where(rng.random(STORE_DIMS) < 0.3, rng.integers(1, 7, STORE_DIMS), rng.integers(-1, 1, STORE_DIMS))
    w[..., 1] = rng.integers(0, 3, STORE_DIMS)
    w[32:40, 16:24, 32:40] = (0, 7)
    w[0:16, 16:24, 0:16] = (0, 1)                         # a second empty chunk: (0, 1, 0)
    return w


def store_ops():
    return [
        op((16, 0, 16), (31, 15, 31), (0, 4)),            # empties chunk (1, 0, 1)
        op((35, 18, 36), (35, 18, 36), (6, 1)),           # fills the empty, clipped chunk (2, 1, 2)
        op((20, 10, 2), (34, 20, 12), (-5, -7)),          # negative ids only (mat != 0: occupied), across chunk borders in x and y
        op((14, 2, 3), (18, 6, 9), (3, 3)),               # two boxes that share cells: the later wins
        op((16, 4, 5), (22, 5, 12), (2, -1)),
        op((3, 17, 3), (3, 17, 3), (0, 9)),               # mat 0 into an empty chunk: it stays empty
    ]
