"""-m "not gpu": the host side of chunk streaming - world_file.stream_view against a direct restatement of WorldManager.LoadChunksAround's
diff and sort (WorldManager.cs:289-370) on a walk of the small world, and the new exports' place in the boundary."""
import math

import numpy as np

from yetanotherconsolegameengine_amd import abi, scenes, world_file
from yetanotherconsolegameengine_amd.scene import Scene

F32 = np.float32
CHUNK, VIEW = 32, 1
WORLD_MIN, VOXEL = (-48.0, 0.0, -48.0), (1.0, 1.0, 1.0)
# crosses a border in x, in z, diagonally, and comes back the same way
PATH = [(0.0, 0.0), (10.0, 0.0), (20.0, 3.0), (40.0, 3.0), (40.0, 20.0), (40.0, 40.0), (5.0, 5.0), (-20.0, -20.0), (-20.0, 10.0), (-20.0, 40.0),
        (5.0, 5.0), (40.0, 40.0), (40.0, 3.0), (0.0, 0.0)]


def _load_chunks_around(prev_desired, loaded_keys, center, chunks_y, non_air):
    """LoadChunksAround on keys alone: (new desired set, keys attached in order, keys removed in order)."""
    sx, sz = F32(F32(VOXEL[0]) * F32(CHUNK)), F32(F32(VOXEL[2]) * F32(CHUNK))
    cxc = int(math.floor(float(F32((F32(center[0]) - F32(WORLD_MIN[0])) / sx))))
    czc = int(math.floor(float(F32((F32(center[2]) - F32(WORLD_MIN[2])) / sz))))
    new = []                                                            # BuildDesiredSet: insertion order of the HashSet
    for cx in range(cxc - VIEW, cxc + VIEW + 1):
        for cz in range(czc - VIEW, czc + VIEW + 1):
            for cy in range(chunks_y):
                new.append((cx, cy, cz))
    new_set, prev_set = set(new), set(prev_desired)
    to_add = [k for k in new if k not in prev_set]
    to_remove = [k for k in prev_desired if k not in new_set]
    to_add.sort(key=lambda k: ((k[0] - cxc) ** 2 + (k[2] - czc) ** 2, k[1]))
    added = [k for k in to_add if k not in loaded_keys and k in non_air]
    removed = [k for k in to_remove if k in loaded_keys]
    return new, added, removed


def test_stream_view_follows_load_chunks_around_on_a_walk_of_the_small_world():
    world = scenes.make_voxel_world(96, 128, 96)
    chunks_y = 128 // CHUNK
    non_air = {(cx, cy, cz) for cx in range(3) for cy in range(chunks_y) for cz in range(3)
               if (world[cx * CHUNK:(cx + 1) * CHUNK, cy * CHUNK:(cy + 1) * CHUNK, cz * CHUNK:(cz + 1) * CHUNK, 0] != 0).any()}
    scene, loaded = Scene(), {}
    want_objects, want_loaded, prev = [], set(), []
    changed, seen_grids = 0, {}
    for x, z in PATH:
        center = (x, 70.0, z)
        added, removed = world_file.stream_view(scene, world, center, WORLD_MIN, VOXEL, CHUNK, VIEW, scenes.VoxelMaterialLookup, loaded)
        prev, w_added, w_removed = _load_chunks_around(prev, want_loaded, center, chunks_y, non_air)
        want_objects += w_added
        want_loaded |= set(w_added)
        for k in w_removed:
            want_objects.remove(k); want_loaded.discard(k)
        assert added == w_added, (x, z)
        assert sorted(removed) == sorted(w_removed), (x, z)
        key_of = {id(v): k for k, v in loaded.items()}
        assert [key_of[id(o)] for o in scene.Objects] == want_objects, (x, z)          # Scene.Objects order after the tick
        assert set(loaded) == want_loaded
        changed += bool(added or removed)
        for k in added:
            vg = loaded[k]
            assert np.array_equal(vg.Cells, world_file.slice_chunk(world, *k, CHUNK))
            assert vg.MinCorner == world_file.chunk_min_corner(WORLD_MIN, VOXEL, CHUNK, *k)
            seen_grids.setdefault(k, []).append(vg)
    assert changed >= 6, changed
    assert any(len(v) >= 2 for v in seen_grids.values())          # the return trip attached again what it had detached


def test_stream_view_reattaches_from_the_cache_the_object_it_cached():
    world = scenes.make_voxel_world(96, 128, 96)
    scene, loaded, cache = Scene(), {}, {}
    world_file.stream_view(scene, world, (0.0, 70.0, 0.0), WORLD_MIN, VOXEL, CHUNK, VIEW, scenes.VoxelMaterialLookup, loaded, cache=cache)
    first = dict(loaded)
    _, removed = world_file.stream_view(scene, world, (40.0, 70.0, 0.0), WORLD_MIN, VOXEL, CHUNK, VIEW, scenes.VoxelMaterialLookup, loaded, cache=cache)
    assert removed and set(cache) == set(removed)
    added, _ = world_file.stream_view(scene, world, (0.0, 70.0, 0.0), WORLD_MIN, VOXEL, CHUNK, VIEW, scenes.VoxelMaterialLookup, loaded, cache=cache)
    assert sorted(added) == sorted(removed) and not cache
    assert all(loaded[k] is first[k] for k in added)          # TryAttachFromCache: the same VolumeGrid comes back


def test_the_streaming_exports_are_part_of_the_boundary():
    assert "ycge_scene_attach_grids" in abi.EXPORTED_SYMBOLS and "ycge_scene_detach_grids" in abi.EXPORTED_SYMBOLS
    assert abi.YCGE_ABI_VERSION == 10          # found by symbol lookup: the version stays
    assert set(abi.HOOK_PROTOTYPES) == {"ycge_debug_read_grid", "ycge_debug_grid_pool_stats", "ycge_debug_peer_context", "ycge_debug_live_resources"}
