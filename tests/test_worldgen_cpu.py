"""Not gpu: the host generator (ycge_worldgen_chunk_cells, csrc/ycge_worldgen.cpp over csrc/ycge_worldgen.h) against the independent numpy
restatement of the reference's C# (tests/worldgen_restatement.py), cell for cell, on a chosen chunk set whose coverage the test asserts."""
import ctypes as C

import numpy as np
import pytest

import worldgen_restatement as R
from yetanotherconsolegameengine_amd import abi

S, CHUNKS_Y = 32, 8
# All from seed 0 (BuildMinecraftLike's).  What each key is in the set for:
CHOSEN = {
    (5, 7, 5): "all air",
    (-2, 1, -2): "wholly underground with Stone metas 0 and 1; negative cx and cz",
    (3, 3, 7): "a lake's edge; 12 trees, conifers and broadleaves; a canopy clipped by the x = 0 face",
    (14, 3, 3): "Desert and Forest columns; a trunk shortened by the chunk's top",
    (14, 3, 75): "the chunk below the next one: surfaces and their trees",
    (14, 4, 75): "columns whose surface lies in the chunk below",
    (330, 1, 0): "beyond IslandRadius: seabed branch, Ocean biome",
    (285, 1, 3): "the fading coast (8200 < distance < 10000 blocks)",
}


def host_chunk(lib, size, chunks_y, seed, key):
    w = abi.World(size, chunks_y, seed, abi.Vec3(0, 0, 0), abi.Vec3(1, 1, 1))
    out = np.full((size, size, size, 2), -9, np.int32)
    any_solid = C.c_int32(-9)
    assert lib.ycge_worldgen_chunk_cells(C.byref(w), *key, out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(any_solid)) == abi.YCGE_OK
    return out, any_solid.value


@pytest.fixture(scope="module")
def chosen():
    cfg = R.Config(S, CHUNKS_Y, 0)
    cols = {}
    out = {}
    for key in CHOSEN:
        col = cols.setdefault((key[0], key[2]), R.columns(key[0], key[2], cfg))
        out[key] = (col, *R.generate_chunk(*key, cfg, col))
    return cfg, out


def test_chosen_set_covers_what_it_is_chosen_for(chosen):
    cfg, set_ = chosen
    assert len(set_) <= 12
    mats = lambda k: set(np.unique(set_[k][1][..., 0]).tolist())
    assert set_[(5, 7, 5)][2] is False and mats((5, 7, 5)) == {R.AIR}
    under = set_[(-2, 1, -2)][1]
    assert mats((-2, 1, -2)) == {R.STONE} and len(np.unique(under[..., 1])) >= 2
    every = set().union(*[mats(k) for k in set_])
    assert {R.WATER, R.SAND, R.DIRT, R.GRASS, R.WOOD, R.LEAVES} <= every
    assert {R.DESERT, R.FOREST} <= set(np.unique(set_[(14, 3, 3)][0]["biome"]).tolist())
    lake = set_[(3, 3, 7)][0]
    assert (lake["water"] > cfg.sea).any() and (lake["biome"] == R.LAKES).any()
    tr = R.trees(lake, 3, cfg)
    assert len(tr) >= 3 and any(t[2] for t in tr) and any(not t[2] for t in tr)
    assert any(t[0] - t[5] < 0 or t[0] + t[5] >= S or t[1] - t[5] < 0 or t[1] + t[5] >= S for t in tr)                 # a canopy clipped by an x or z face
    assert any(t[6] > S - 1 for t in R.trees(set_[(14, 3, 3)][0], 3, cfg))                                                 # desiredTop > size - 1
    below = R.trees(set_[(14, 3, 75)][0], 3, cfg)
    assert below and all((t[0], t[1]) not in {(u[0], u[1]) for u in R.trees(set_[(14, 4, 75)][0], 4, cfg)} for t in below)  # the chunk above gets none of them
    assert (set_[(330, 1, 0)][0]["biome"] == R.OCEAN).all() and 330 * S >= 10000
    assert 8200 < 285 * S < 10000


def test_host_export_equals_the_restatement_on_the_chosen_set(product_lib, chosen):
    cfg, set_ = chosen
    for key, (col, ref, any_ref) in set_.items():
        got, any_got = host_chunk(product_lib, S, CHUNKS_Y, 0, key)
        assert int((got != ref).sum()) == 0, key
        assert any_got == int(any_ref), key


@pytest.mark.parametrize("size,chunks_y,seed,key", [(8, 8, 3, (100, 2, -100)), (12, 8, 0, (10, 3, 4)), (64, 4, 0, (1, 1, 1))])
def test_host_export_equals_the_restatement_at_other_chunk_sizes(product_lib, size, chunks_y, seed, key):
    cfg = R.Config(size, chunks_y, seed)
    ref, any_ref = R.generate_chunk(*key, cfg)
    got, any_got = host_chunk(product_lib, size, chunks_y, seed, key)
    assert int((got != ref).sum()) == 0 and any_got == int(any_ref)


def test_height_y_along_a_line_is_what_the_host_fills(product_lib):
    cfg = R.Config(S, CHUNKS_Y, 0)
    gx = np.arange(14 * S, 15 * S)
    h = R.height_y(gx, np.full_like(gx, 3 * S + 5), cfg)
    for cy in range(CHUNKS_Y):
        got, _ = host_chunk(product_lib, S, CHUNKS_Y, 0, (14, cy, 3))
        col_solid = got[:, :, 5, 0]
        for lx in range(S):
            top = h[lx] - cy * S
            if 0 <= top < S:
                assert col_solid[lx, top] not in (R.AIR, R.WATER) and (top + 1 >= S or col_solid[lx, top + 1] in (R.AIR, R.WATER, R.WOOD, R.LEAVES))


def test_refusals(product_lib):
    out = np.zeros(2 * 65 ** 3, np.int32)
    p, a = out.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(0)
    for size in (3, 65):
        w = abi.World(size, 8, 0, abi.Vec3(0, 0, 0), abi.Vec3(1, 1, 1))
        assert product_lib.ycge_worldgen_chunk_cells(C.byref(w), 0, 0, 0, p, C.byref(a)) == abi.YCGE_ERR_INVALID_ARG
    w = abi.World(8, 8, 0, abi.Vec3(0, 0, 0), abi.Vec3(1, 1, 1))
    assert product_lib.ycge_worldgen_chunk_cells(None, 0, 0, 0, p, C.byref(a)) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_worldgen_chunk_cells(C.byref(w), 0, 0, 0, None, C.byref(a)) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_worldgen_chunk_cells(C.byref(w), 0, 0, 0, p, None) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_abi_sizeof(11) == C.sizeof(abi.World)
    # keys outside +-2^24 blocks (not exact in binary32): refused as ycge_scene_generate_grids refuses them
    lim = (1 << 24) // 8
    for key in ((lim + 1, 0, 0), (0, -lim - 1, 0), (0, 0, 2 ** 31 - 1)):
        assert product_lib.ycge_worldgen_chunk_cells(C.byref(w), *key, p, C.byref(a)) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_worldgen_chunk_cells(C.byref(w), lim, 0, -lim, p, C.byref(a)) == abi.YCGE_OK


def test_stream_generated_orders_attaches_and_returns_what_left():
    """world_file.stream_generated against a stub renderer: the reference's attach order (radial distance, then cy), -1 kept as loaded,
    the keys that left returned with the indices to detach."""
    from yetanotherconsolegameengine_amd import world_file

    class Stub:
        def __init__(self):
            self.calls, self.next = [], 0

        def GenerateGrids(self, world, keys, proto):
            self.calls.append(list(keys))
            out = []
            for k in keys:
                if k[1] >= 6:
                    out.append(-1)
                else:
                    out.append(self.next); self.next += 1
            return out

    world = abi.World(32, 8, 0, abi.Vec3(-512, 0, -512), abi.Vec3(1, 1, 1))
    r, loaded = Stub(), {}
    added, removed, gone = world_file.stream_generated(r, world, None, (0.0, 120.0, 0.0), 1, loaded)
    assert removed == [] and gone == [] and len(added) == 9 * 8 == len(loaded) and r.calls == [added]
    d = [(k[0] - 16) ** 2 + (k[2] - 16) ** 2 for k in added]
    assert d == sorted(d) and added[:8] == [(16, cy, 16) for cy in range(8)]          # the centre column first, cy ascending (WorldManager.cs:313-320)
    assert sorted(added) == sorted(world_file.build_desired_set((0.0, 120.0, 0.0), (-512, 0, -512), (1, 1, 1), 32, 1, 8))
    assert all((loaded[k] == -1) == (k[1] >= 6) for k in added)
    before = dict(loaded)
    added2, removed2, gone2 = world_file.stream_generated(r, world, None, (33.0, 120.0, 0.0), 1, loaded)          # one column to +x
    assert sorted(removed2) == sorted(k for k in before if k[0] == 15) and sorted(gone2) == sorted(before[k] for k in removed2 if before[k] >= 0)
    assert sorted(added2) == [(18, cy, cz) for cy in range(8) for cz in (15, 16, 17)] or sorted(added2) == sorted((18, cy, cz) for cz in (15, 16, 17) for cy in range(8))
    assert len(loaded) == 72 and r.calls[-1] == added2
    assert world_file.stream_generated(r, world, None, (33.0, 120.0, 0.0), 1, loaded) == ([], [], []) and len(r.calls) == 2
