"""Not gpu: the host generator of the pregenerated world (ycge_worldgen_world_cells, csrc/ycge_worldgen.cpp over csrc/ycge_worldgen.h) and
its hooks against the numpy restatement of WorldManager.GenerateAndSaveWorld (tests/worldpregen_restatement.py), cell for cell, on windows
whose coverage the first test asserts.

The windows were found by profiles/worldpregen_windows.py (a CPU search over origins and seeds with the restatement) and are pinned here.
Two cases of the list, and which way each went:
  * a tree with anyLeaves == false was FOUND in natural terrain (window "fallback": a tree whose whole canopy earlier trees had taken), so
    the fallback crown and the fixed-point passes are tested on a real window, not on synthetic fields;
  * a tree clipped at the world's top (FloraPlacer.cs:168-169) was NOT found and is, as far as the search goes, not there to find: the clip
    needs ground within 16 of the top (trunkBase + trunkH + 2 >= ny, trunkH <= 13) and ground never exceeds sea + 0.45 ny = 0.7 ny, so
    ny <= 53.  Worlds that low do have land, but only LOW land: LocalWaterY's lake candidate, sea + 8 + 60 * (0.75 lakeField + 0.25
    lowlandBias), lies above all the higher ground, so every column near the top is Lakes and carries no tree (no column of a 125-block
    grid over the island is land with ground >= ny - 16 at ny <= 48, seeds 0..6).  This is a DEPARTURE from the list of cases the windows
    were to cover: the clip is tested on synthetic fields through ycge_host_worldgen_world_from_fields
    (test_top_clip_on_synthetic_fields), on the host only - no window and no device test reaches feature_at's clip branch.

FOREST4 is the "forest" window cut into chunks of 4 (the same cells: height, seed and origin are unchanged).  Chunks that small fit between
a column's ground and a neighbouring tree's canopy: all Air with occupied chunks below AND above in the same chunk column, which a rule
"occupied up to the column's top" gets wrong (test_chunks_of_four_leave_air_chunks_under_canopies; the device case is in
tests/test_gpu_worldpregen.py)."""
import ctypes as C

import numpy as np
import pytest

import worldgen_restatement as R
import worldpregen_restatement as P
from yetanotherconsolegameengine_amd import abi, world_file

# name: (chunk_size, chunks_y, chunks_x, chunks_z, seed, origin_bx, origin_bz)
WINDOWS = {
    "forest": (16, 8, 4, 4, 0, -8532, 218),          # both tree kinds, canopies across chunk borders in x, y, z, overlapping canopies, a canopy cut by the window's edge, the 3.5 bank rule, a lake
    "fallback": (12, 10, 5, 4, 0, -8155, -4024),     # a tree with anyLeaves == false; cacti and rock piles
    "small": (8, 14, 5, 4, 3, -8020, -1766),         # chunks of 8, another seed: trees, desert, lake
    "shore": (12, 10, 3, 3, 7, -10143, -518),        # the ocean; an edge whose clamped slope differs
    "origin": (32, 8, 4, 4, 0, 0, 0),                # the reference's own window: Lakes with Forest and Desert columns
}


FOREST4 = (4, 32, 16, 16, 0, -8532, 218)


def bind(lib):
    for name, (res, args) in abi.WORLDGEN_HOOK_PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def world_of(S, chunks_y, seed, world_min=(0, 0, 0)):
    return abi.World(S, chunks_y, seed, abi.Vec3(*world_min), abi.Vec3(1, 1, 1))


def host_world(lib, S, chunks_y, chunks_x, chunks_z, seed, ox, oz):
    out = np.full((chunks_x * S, chunks_y * S, chunks_z * S, 2), -9, np.int32)
    assert lib.ycge_worldgen_world_cells(C.byref(world_of(S, chunks_y, seed)), chunks_x, chunks_z, ox, oz, out.ctypes.data_as(C.POINTER(C.c_int32))) == abi.YCGE_OK
    return out


def host_fields(lib, S, chunks_y, chunks_x, chunks_z, seed, ox, oz):
    bind(lib)
    nx, nz = chunks_x * S, chunks_z * S
    i32 = lambda: np.full((nx, nz), -9, np.int32)
    f = dict(ground0=i32(), ground=i32(), dir=i32(), accum=np.full((nx, nz), -9, np.float32), slope=np.full((nx, nz), -9, np.float32), biome=i32(), water=i32(),
             feature=np.zeros((nx, nz), np.uint32), climate=i32(), rock=i32())
    assert lib.ycge_host_worldgen_world_fields(C.byref(world_of(S, chunks_y, seed)), chunks_x, chunks_z, ox, oz, *[f[k].ctypes.data for k in
                                               ("ground0", "ground", "dir", "accum", "slope", "biome", "water", "feature", "climate", "rock")]) == abi.YCGE_OK
    return f


_REF = {}


def reference(name):
    """(cfg, cells, fields, placed) of a window by the restatement: computed once, shared (tests/test_gpu_worldpregen.py does not need it)."""
    if name not in _REF:
        S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
        cfg = R.Config(S, cy, seed)
        _REF[name] = (cfg, *P.generate_world(cfg, cx, cz, ox, oz))
    return _REF[name]


def test_chosen_windows_cover_what_they_were_chosen_for():
    tags = {}
    for name, (S, cy, cx, cz, seed, ox, oz) in WINDOWS.items():
        assert (name == "origin" and S == 32) or (S in (8, 12, 16) and 3 <= cx <= 6 and 3 <= cz <= 6)
        cfg, cells, f, placed = reference(name)
        tags[name] = P.window_tags(cfg, cells, f, placed, ox, oz)
    every = set().union(*tags.values())
    assert every >= set(P.TAGS) - {"top_clip"}, sorted(set(P.TAGS) - every)          # (top_clip: see the module's docstring)
    assert "no_leaves" in tags["fallback"] and "ocean" in tags["shore"] and {"cross_x", "cross_y", "cross_z", "overlap", "edge_clip", "beach35"} <= tags["forest"]
    assert {R.FOREST, R.DESERT} <= set(np.unique(reference("origin")[2]["biome"]).tolist())
    cfg, cells, f, placed = reference("forest")
    # the 3.5 bank rule where the per-chunk rule (<= 2) would not: a ground cell of Sand under wY - gY == 3 whose surface block would be something else
    d = f["water"] - f["ground"]
    bank = (f["water"] > cfg.sea) & (d == 3) & (np.abs(f["ground"] - cfg.sea) > 2) & (f["ground"] < cfg.snow) & (f["biome"] != R.DESERT)
    assert bank.any()
    x, z = np.argwhere(bank)[0]
    assert cells[x, f["ground"][x, z], z, 0] == R.SAND
    # a rock pile's (Stone, 1) in a neighbouring column, a cactus of Wood on Sand
    fb = reference("fallback")
    assert fb[3]["cacti"] and fb[3]["rocks"] and any(not t[7] for t in fb[3]["trees"])


def test_chunks_of_four_leave_air_chunks_under_canopies(product_lib):
    S = FOREST4[0]
    assert FOREST4[0] * FOREST4[1] == WINDOWS["forest"][0] * WINDOWS["forest"][1] and FOREST4[4:] == WINDOWS["forest"][4:]
    cfg, ref, f, placed = reference("forest")
    got = host_world(product_lib, *FOREST4)
    assert got.tobytes() == ref.tobytes()          # the cells do not depend on how the window is cut into chunks
    occ = P.chunk_occupied(ref, S)
    below = np.maximum.accumulate(occ, axis=1)                          # occupied at or below (cumulative from cy = 0 up) ...
    above = np.maximum.accumulate(occ[:, ::-1], axis=1)[:, ::-1]        # ... and at or above
    gaps = ~occ & above
    assert gaps.sum() >= 5 and below[gaps].all()          # all-Air chunks with something above them (cy = 0 is always occupied below)
    cx, cy, cz = np.argwhere(gaps)[0]
    block = ref[cx * S:(cx + 1) * S, :, cz * S:(cz + 1) * S, 0]
    assert (block[:, cy * S:(cy + 1) * S] == R.AIR).all() and np.isin(block[:, (cy + 1) * S:], (R.LEAVES, R.WOOD)).any()          # what is above is a tree


@pytest.mark.parametrize("name", list(WINDOWS))
def test_world_cells_equal_the_restatement(product_lib, name):
    cfg, ref, f, placed = reference(name)
    got = host_world(product_lib, *WINDOWS[name])
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), int((got != ref).sum())


@pytest.mark.parametrize("name", list(WINDOWS))
def test_fields_hook_equals_the_restatement(product_lib, name):
    cfg, ref, f, placed = reference(name)
    h = host_fields(product_lib, *WINDOWS[name])
    for k in ("ground0", "ground", "dir", "biome", "water", "climate", "rock"):
        assert (h[k] == f[k]).all(), k
    assert h["accum"].tobytes() == f["accum"].astype(np.float32).tobytes()          # against the literal ascending sort
    assert h["slope"].tobytes() == f["slope"].astype(np.float32).tobytes()
    assert float(h["accum"].max()) <= 8.0 and (h["ground"] == h["ground0"]).all()          # far from RiverAccumThreshold: nothing is carved
    # the descriptors name the features the serial loops placed, with their sizes
    kind = h["feature"] & 3
    assert sorted(map(tuple, np.argwhere(kind == 1))) == sorted((t[0], t[1]) for t in placed["trees"])
    assert sorted(map(tuple, np.argwhere(kind == 2))) == sorted((c[0], c[1]) for c in placed["cacti"])
    assert sorted(map(tuple, np.argwhere(kind == 3))) == sorted(placed["rocks"])
    for gx, gz, conifer, base, th, r, clipped, any_leaves in placed["trees"]:
        d = int(h["feature"][gx, gz])
        assert ((d >> 2) & 1, (d >> 3) & 31, (d >> 8) & 3) == (int(conifer), th, r)
    for gx, gz, height in placed["cacti"]:
        assert (int(h["feature"][gx, gz]) >> 3) & 7 == height


def river(lib, ground, sea):
    bind(lib)
    g = np.ascontiguousarray(ground, np.int32)
    nx, nz = g.shape
    d, a, c, w = np.zeros((nx, nz), np.int32), np.zeros((nx, nz), np.float32), np.zeros((nx, nz), np.int32), np.zeros((nx, nz), np.int32)
    assert lib.ycge_host_worldgen_river_global(g.ctypes.data, nx, nz, sea, d.ctypes.data, a.ctypes.data, c.ctypes.data, w.ctypes.data) == abi.YCGE_OK
    return d, a, c, w


def test_river_accum_against_the_literal_sort_with_many_ties(product_lib):
    rng = np.random.default_rng(11)
    for shape, levels in (((23, 17), 3), ((9, 31), 2), ((1, 12), 4), ((14, 1), 3), ((30, 30), 40)):
        ground = rng.integers(10, 10 + levels, shape).astype(np.int64)          # few levels: most neighbours tie
        dnx, dnz = P.d8_global(ground)
        d, a, c, w = river(product_lib, ground, 8)
        assert (d == (dnx + 1) * 3 + (dnz + 1)).all()
        for rev in (False, True):          # Array.Sort is unstable: either order among equal heights
            assert a.tobytes() == P.accum_sorted(ground, dnx, dnz, reverse_ties=rev).tobytes(), (shape, rev)
        assert (c == ground).all() and (w == 8).all()


def test_a_pit_with_eight_neighbours_counts_eight(product_lib):
    ground = np.full((5, 5), 20, np.int64)
    ground[2, 2] = 10          # the pit: all eight neighbours drain into it; it has no lower neighbour itself and adds nothing (RiverNetworkGlobal.cs:58)
    d, a, c, w = river(product_lib, ground, 8)
    assert a[2, 2] == 8.0 and d[2, 2] == 4 and a.sum() == 8.0
    assert a.tobytes() == P.accum_sorted(ground, *P.d8_global(ground)).tobytes()
    # the per-chunk pass counts the pit itself as well: 9 (csrc/ycge_worldgen.h, river_accum)
    tile = np.full((7, 7), 20, np.int32); tile[3, 3] = 10
    lib = product_lib
    lib.ycge_host_worldgen_river.restype = C.c_int
    lib.ycge_host_worldgen_river.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
    d5, a5, c5, w5 = np.zeros(25, np.int32), np.zeros(25, np.float32), np.zeros(25, np.int32), np.zeros(25, np.int32)
    assert lib.ycge_host_worldgen_river(tile.ctypes.data, 5, 8, d5.ctypes.data, a5.ctypes.data, c5.ctypes.data, w5.ctypes.data) == abi.YCGE_OK
    assert a5.reshape(5, 5)[2, 2] == 9.0


def test_the_window_moves_with_the_origin(product_lib):
    S, cy, seed = 8, 14, 3
    big = host_fields(product_lib, S, cy, 6, 6, seed, -8040, -1790)
    for (a, b) in ((8, 16), (16, 0), (0, 24)):
        sub = host_fields(product_lib, S, cy, 3, 3, seed, -8040 + a, -1790 + b)
        for k in ("ground0", "climate", "rock"):
            assert (sub[k] == big[k][a:a + 24, b:b + 24]).all(), (a, b, k)
    # ... and nothing else: the edge clamps are the window's own (a column on the small window's edge sees no neighbour beyond it)
    sub = host_fields(product_lib, S, cy, 3, 3, seed, -8040 + 8, -1790 + 16)
    cfg = R.Config(S, cy, seed)
    f = P.fields(cfg, 24, 24, -8040 + 8, -1790 + 16)
    assert (sub["dir"] == f["dir"]).all() and sub["slope"].tobytes() == f["slope"].astype(np.float32).tobytes()


@pytest.mark.parametrize("name", ["forest", "fallback", "small"])
def test_the_gather_equals_the_serial_loops(product_lib, name):
    """The kernels' scheme (csrc/ycge_worldpregen.hip) run on the host: fallback flags to their fixed point, then every cell by one gather."""
    lib = bind(product_lib)
    S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
    cfg, ref, f, placed = reference(name)
    h = host_fields(lib, *WINDOWS[name])
    out, passes = np.full(ref.shape, -9, np.int32), C.c_int32(-1)
    args = [np.ascontiguousarray(h[k]) for k in ("ground", "water", "slope", "biome", "rock", "feature")]
    assert lib.ycge_host_worldgen_world_from_fields(C.byref(world_of(S, cy, seed)), cx * S, cz * S, *[a.ctypes.data for a in args], 1, out.ctypes.data, C.byref(passes)) == abi.YCGE_OK
    assert out.tobytes() == ref.tobytes()
    no_leaves = sum(1 for t in placed["trees"] if not t[7])
    assert passes.value >= 2 if no_leaves else passes.value == 1          # a flag flipped: at least one more pass to see that nothing else does


def test_top_clip_on_synthetic_fields(product_lib):
    """FloraPlacer.cs:168-169 (see the module's docstring for why no natural window has it): a Forest plateau two to four below SnowLevel - 2
    in a world 32 high, trees where the hash puts them; serial loops and gather against the restatement's loops on the same fields."""
    lib = bind(product_lib)
    S, cy, nx, nz = 8, 4, 40, 24
    cfg = R.Config(S, cy, 5)
    rng = np.random.default_rng(2)
    f = dict(ground=rng.integers(19, 23, (nx, nz)).astype(np.int64), water=np.full((nx, nz), cfg.sea, np.int64), slope=np.zeros((nx, nz), np.float32),
             biome=np.full((nx, nz), R.FOREST, np.int64), rock_n=np.full((nx, nz), 0.5, np.float32))
    assert cfg.height == 32 and f["ground"].max() < cfg.snow - 2
    ref = P.fill(cfg, f)
    placed = P.place_trees_global(cfg, f, ref)
    clipped = [t for t in placed["trees"] if t[6]]
    assert len(clipped) >= 3 and any(t[2] for t in clipped) and any(not t[2] for t in clipped) and any(not t[6] for t in placed["trees"])
    assert any(t[3] + t[4] + 2 == cfg.height and t[4] > 3 for t in clipped)          # trunkH = ny - trunkBase - 2 took effect
    ins = [np.ascontiguousarray(f["ground"], np.int32), np.ascontiguousarray(f["water"], np.int32), f["slope"], np.ascontiguousarray(f["biome"], np.int32),
           np.ones((nx, nz), np.int32)]
    for gather in (0, 1):
        out, passes = np.full(ref.shape, -9, np.int32), C.c_int32(-1)
        assert lib.ycge_host_worldgen_world_from_fields(C.byref(world_of(S, cy, 5)), nx, nz, *[a.ctypes.data for a in ins], None, gather, out.ctypes.data, C.byref(passes)) == abi.YCGE_OK
        assert out.tobytes() == ref.tobytes(), gather


def test_refusals_leave_cells_out_untouched(product_lib):
    lib = product_lib
    out = np.full(2 * 16 * 32 * 16, -9, np.int32)
    p = out.ctypes.data_as(C.POINTER(C.c_int32))
    ok = world_of(8, 4, 0)
    call = lambda w, cx, cz, ox, oz, dst=p: lib.ycge_worldgen_world_cells(C.byref(w) if w is not None else None, cx, cz, ox, oz, dst)
    for size in (3, 65):          # what worldgen_check refuses
        assert call(world_of(size, 4, 0), 2, 2, 0, 0) == abi.YCGE_ERR_INVALID_ARG
    assert call(world_of(8, 0, 0), 2, 2, 0, 0) == abi.YCGE_ERR_INVALID_ARG
    assert call(None, 2, 2, 0, 0) == abi.YCGE_ERR_INVALID_ARG
    for cx, cz in ((0, 2), (2, 0), (-1, 2)):
        assert call(ok, cx, cz, 0, 0) == abi.YCGE_ERR_INVALID_ARG
    lim = 1 << 24
    for ox, oz in ((lim - 14, 0), (0, lim - 14), (-lim - 1, 0), (0, -lim - 1), (2 ** 31 - 1, 0)):          # a window whose block coordinates leave +-2^24
        assert call(ok, 2, 2, ox, oz) == abi.YCGE_ERR_INVALID_ARG
    assert call(world_of(64, 16, 0), 16, 16, 0, 0) == abi.YCGE_ERR_INVALID_ARG          # 1024^3 = 2^30 cells
    assert call(world_of(64, 16, 0), 2 ** 20, 2 ** 20, 0, 0) == abi.YCGE_ERR_INVALID_ARG
    assert call(ok, 2, 2, 0, 0, None) == abi.YCGE_ERR_INVALID_ARG
    assert (out == -9).all()
    assert call(ok, 2, 2, lim - 15, -lim) == abi.YCGE_OK and (out != -9).all()          # the last block is 2^24: still exact in binary32


def test_pregen_world_round_trip(product_lib, tmp_path):
    S, cy, cx, cz, seed, ox, oz = WINDOWS["shore"]
    path = tmp_path / "world.vg01"
    cells = world_file.pregen_world(product_lib, world_of(S, cy, seed), cx, cz, path, origin=(ox, oz))
    back = world_file.read_vg01(path)
    assert back.shape == (cx * S, cy * S, cz * S, 2) and back.tobytes() == cells.tobytes() == reference("shore")[1].tobytes()
    assert path.stat().st_size == 16 + cells.nbytes
    with pytest.raises(ValueError):
        world_file.pregen_world(product_lib, world_of(S, cy, seed), 0, cz)


def test_the_exports_are_declared_everywhere():
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    header, hooks, cs = (root / "include" / "ycge.h").read_text(), (root / "include" / "ycge_hooks.h").read_text(), (root / "bindings" / "csharp" / "Ycge.cs").read_text()
    for name in ("ycge_worldgen_world_cells", "ycge_scene_generate_world"):
        assert ("int " + name + "(") in header and name in abi._PROTOTYPES and ("int " + name + "(") in cs and ("int " + name + "(") not in hooks
    for name in ("ycge_host_worldgen_world_fields", "ycge_host_worldgen_world_from_fields", "ycge_host_worldgen_river_global", "ycge_debug_worldpregen_stats"):
        assert ("int " + name + "(") in hooks and name in abi.WORLDGEN_HOOK_PROTOTYPES and ("int " + name + "(") not in header
    assert "#define YCGE_ABI_VERSION 10" in header and abi.YCGE_ABI_VERSION == 10
    assert "is not offered" not in header and "Not restated: the whole-world" not in (root / "yetanotherconsolegameengine_amd" / "csrc" / "ycge_worldgen.h").read_text()
