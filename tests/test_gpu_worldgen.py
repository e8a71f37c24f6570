"""-m gpu: ycge_scene_generate_grids (csrc/ycge_worldgen_scene.cpp over csrc/ycge_worldgen.hip) against the host generator
(ycge_worldgen_chunk_cells) - raw cells byte for byte, indices, and frames and queries bit for bit against a twin context that attaches the
host generator's cells with ycge_scene_attach_grids.  The chunk set is tests/test_worldgen_cpu.py's, which asserts what it covers."""
import ctypes as C
import os

import numpy as np
import pytest

import parity_util as pu
from test_worldgen_cpu import CHOSEN, CHUNKS_Y, S, host_chunk
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import AmbientLight, Material, Scene, Sphere, ZERO, flatten, vec3

pytestmark = pytest.mark.gpu

AIR_KEY = (5, 7, 5)
# the chosen set in one batch: two cy of (14, *, 75) are in it; (3, 3, 7) is named twice
KEYS = list(CHOSEN) + [(3, 3, 7)]
FRAME_BUFFERS = (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY, abi.BUF_PREV_NORMAL,
                 abi.BUF_PREV_DEPTH, abi.BUF_PREV_SKY, abi.BUF_DENOISED)
WORLD_MIN = (-512.0, 0.0, -512.0)


def _world(size=S, chunks_y=CHUNKS_Y, seed=0):
    return abi.World(size, chunks_y, seed, abi.Vec3(*WORLD_MIN), abi.Vec3(1, 1, 1))


def _anchor():
    """A lit scene (sun and moon) with 27 materials and no grid: what the chunks are generated into."""
    rng = np.random.default_rng(3)
    s = Scene()
    s.IsVolumeScene = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.0)
    lights, top, bottom = scenes.sun_moon_lights(0.4)
    s.Lights.extend(lights)
    s.BackgroundTop, s.BackgroundBottom = top, bottom
    for _ in range(27):
        s.Add(Sphere(vec3(0, -500, 0), 0.1, Material(vec3(*rng.uniform(0.1, 0.9, 3)), 0.1, 0.0, ZERO)))
    return flatten(s)


def _proto(lookup_pairs, default_material=-1):
    lk = (abi.VoxelLookup * len(lookup_pairs))(*[abi.VoxelLookup(a, b, (a * 3 + b) % 27) for a, b in lookup_pairs])
    g = abi.Grid()
    g.lookup, g.n_lookup, g.default_material = C.cast(lk, C.POINTER(abi.VoxelLookup)), len(lookup_pairs), default_material
    g.wireframe, g.wire_width_fraction, g.wire_max_distance = 1, 0.06, 16.0
    g.voxel_size = abi.Vec3(1, 1, 1)
    return g, lk


ALL_PAIRS = [(m, k) for m in range(1, 9) for k in range(3)]


def _host_cells(lib, world, keys):
    return np.stack([host_chunk(lib, world.chunk_size, world.chunks_y, world.world_seed, k)[0] for k in keys])


@pytest.fixture(scope="module")
def host_set(product_lib):
    return _host_cells(product_lib, _world(), KEYS)


def _same(a, b, label):
    assert a.shape == b.shape, label
    n = pu.mismatch_count(a, b)
    assert n == 0, f"{label}: {n} elements differ"


def test_cells_and_indices_of_the_chosen_set_in_one_call(product_lib, host_set):
    r = RaytraceRenderer(_anchor(), 32, 16)
    proto, keep = _proto(ALL_PAIRS)
    idx, cells = r.GenerateGrids(_world(), KEYS, proto, want_cells=True)
    assert cells.tobytes() == host_set.tobytes()
    air = KEYS.index(AIR_KEY)
    assert idx[air] == -1 and [i for k, i in enumerate(idx) if k != air] == list(range(len(KEYS) - 1))          # no slot for the all-air chunk, lowest free first
    st, wg = r.grid_pool_stats(), r.worldgen_stats()
    assert st["resident"] == len(KEYS) - 1 and wg["device_chunks"] == len(KEYS) and wg["host_chunks"] == 0
    r.close()


@pytest.mark.parametrize("size,chunks_y,seed,keys", [(8, 8, 3, [(100, 2, -100), (100, 3, -100), (0, 1, 0)]), (12, 8, 0, [(10, 3, 4), (10, 7, 4), (-3, 2, 5)]),
                                                     (64, 4, 0, [(1, 1, 1), (1, 3, 1), (-2, 1, 0)])])
def test_cells_at_other_chunk_sizes(product_lib, size, chunks_y, seed, keys):
    w = _world(size, chunks_y, seed)
    r = RaytraceRenderer(_anchor(), 32, 16)
    proto, keep = _proto(ALL_PAIRS)
    idx, cells = r.GenerateGrids(w, keys, proto, want_cells=True)
    assert cells.tobytes() == _host_cells(product_lib, w, keys).tobytes()
    r.close()


def _solid_keys():
    return [k for k in KEYS if k != AIR_KEY]


def _prims(idx):
    arr = (abi.Prim * len(idx))()
    for j, i in enumerate(idx):
        arr[j].type, arr[j].ref, arr[j].material = abi.PRIM_VOLUME_GRID, i, 0
    return arr


def _attach_host(r, lib, world, keys, proto):
    cells = _host_cells(lib, world, keys)
    recs = (abi.Grid * len(keys))()
    for j, k in enumerate(keys):
        C.memmove(C.byref(recs[j]), C.byref(proto), C.sizeof(abi.Grid))
        recs[j].nx = recs[j].ny = recs[j].nz = world.chunk_size
        recs[j].min_corner = abi.Vec3(*[np.float32(WORLD_MIN[a]) + np.float32(k[a] * world.chunk_size) * np.float32(1) for a in range(3)])
        recs[j].cells = cells[j].ctypes.data_as(C.POINTER(C.c_int32))
    out = (C.c_int32 * len(keys))()
    r._check(r.L.ycge_scene_attach_grids(r.ctx, recs, len(keys), out))
    return [int(i) for i in out]


def _pose_over(key):
    return (WORLD_MIN[0] + key[0] * S + 16.0, 140.0, WORLD_MIN[2] + key[2] * S + 16.0)          # above the chunk's middle


def _frames_and_hits(r, idx, label, other=None):
    arr = _prims(idx)
    r._check(r.L.ycge_scene_update_objects(r.ctx, arr, len(idx)))
    out = []
    r.SetCamera(_pose_over((3, 3, 7)), 0.0, -1.2)
    for f in range(3):
        r.TryFlipAndBlit(want_sdr=True)
        out.append([r.read(which) for which in FRAME_BUFFERS])
    rng = np.random.default_rng(9)
    o = np.tile(np.asarray(_pose_over((3, 3, 7)), np.float32), (256, 1))
    d = rng.normal(size=(256, 3)).astype(np.float32); d[:, 1] = -np.abs(d[:, 1]) - 0.3
    out.append(list(r.Hit(o, d)))
    return out


@pytest.mark.parametrize("in_flight", [0, 2])
def test_frames_and_queries_equal_an_attach_of_the_host_cells(product_lib, in_flight):
    keys, world = _solid_keys(), _world()
    proto, keep = _proto(ALL_PAIRS)
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    for r in (A, B):
        r.SetCamera(_pose_over((3, 3, 7)), 0.0, -1.2)
        for _ in range(in_flight):
            r.RenderAsync()
    ia = A.GenerateGrids(world, keys, proto)
    ib = _attach_host(B, product_lib, world, keys, proto)
    assert ia == ib
    fa, fb = _frames_and_hits(A, ia, "generated"), _frames_and_hits(B, ib, "attached")
    for f, (x, y) in enumerate(zip(fa, fb)):
        for w, (p, q) in enumerate(zip(x, y)):
            _same(np.asarray(p), np.asarray(q), f"frame / query {f}, buffer {w}")
    assert (np.asarray(fa[3][1])[:, 0] >= 0).any()          # (the downward rays do meet the chunks)
    A.close(); B.close()


def _replay(r, idx):
    """the same 3 frames and hit batch from the same start: frame counter 0, the TAA history dropped (ycge_resize does), the same pose"""
    r._check(r.L.ycge_resize(r.ctx, r.fbW, r.fbH, r.ss))
    r._check(r.L.ycge_set_frame_counter(r.ctx, 0))
    return _frames_and_hits(r, idx, "replay")


def test_refusals_leave_the_scene_as_it_was(product_lib):
    L = product_lib
    keys, world = _solid_keys()[:3], _world()
    proto, keep = _proto(ALL_PAIRS)
    r = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    idx = r.GenerateGrids(world, keys, proto)
    before = _replay(r, idx)
    pool = r.grid_pool_stats()
    karr = np.ascontiguousarray(np.asarray(_solid_keys()[3:6], np.int32))
    kp = karr.ctypes.data_as(C.POINTER(C.c_int32))
    out = (C.c_int32 * 3)(-7, -7, -7)

    def unchanged(label):
        assert list(out) == [-7, -7, -7], label
        st = r.grid_pool_stats()
        assert (st["resident"], st["arena_in_use"], st["free_indices"]) == (pool["resident"], pool["arena_in_use"], pool["free_indices"]), label
        after = _replay(r, idx)          # renderable, and the same frames and hits as before the refusal, bit for bit
        for f, (x, y) in enumerate(zip(before, after)):
            for w, (p, q) in enumerate(zip(x, y)):
                _same(np.asarray(p), np.asarray(q), f"{label}: frame / query {f}, buffer {w}")

    for size in (3, 65):
        assert L.ycge_scene_generate_grids(r.ctx, C.byref(_world(size)), kp, 3, C.byref(proto), out, None) == abi.YCGE_ERR_INVALID_ARG
    unchanged("bad chunk size")
    few, keep2 = _proto([(1, 0)], default_material=-1)          # the chunks hold more pairs than this lookup
    assert L.ycge_scene_generate_grids(r.ctx, C.byref(world), kp, 3, C.byref(few), out, None) == abi.YCGE_ERR_INVALID_ARG
    assert b"no material" in L.ycge_last_error(r.ctx)
    unchanged("a pair with no material")
    # ... the same refusal with two frames in flight: it comes from inside the encode, after the frames were joined
    r._check(L.ycge_resize(r.ctx, r.fbW, r.fbH, r.ss)); r._check(L.ycge_set_frame_counter(r.ctx, 0))
    r.SetCamera(_pose_over((3, 3, 7)), 0.0, -1.2)
    r.RenderAsync(); r.RenderAsync()
    assert L.ycge_scene_generate_grids(r.ctx, C.byref(world), kp, 3, C.byref(few), out, None) == abi.YCGE_ERR_INVALID_ARG
    r.Wait()
    unchanged("a pair with no material, frames in flight")
    empty = RaytraceRenderer(None, 32, 16)
    assert L.ycge_scene_generate_grids(empty.ctx, C.byref(world), kp, 3, C.byref(proto), out, None) == abi.YCGE_ERR_NO_SCENE and list(out) == [-7, -7, -7]
    empty.close()
    # a later generate takes the next indices
    assert r.GenerateGrids(world, _solid_keys()[3:6], proto) == [3, 4, 5]
    r.close()


def test_the_host_knob_gives_the_same_cells_and_frames(product_lib, host_set):
    keys, world = _solid_keys(), _world()
    proto, keep = _proto(ALL_PAIRS)
    os.environ["YCGE_WORLDGEN_HOST"] = "1"
    try:
        H = RaytraceRenderer(_anchor(), 96, 27, 60.0)          # (knobs are read when the context is made)
    finally:
        del os.environ["YCGE_WORLDGEN_HOST"]
    D = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    ih, ch = H.GenerateGrids(world, KEYS, proto, want_cells=True)
    id_, cd = D.GenerateGrids(world, KEYS, proto, want_cells=True)
    assert ih == id_ and ch.tobytes() == cd.tobytes() == host_set.tobytes()
    assert H.worldgen_stats()["host_chunks"] == len(KEYS) and D.worldgen_stats()["device_chunks"] == len(KEYS)
    fh, fd = _frames_and_hits(H, [i for i in ih if i >= 0], "host knob"), _frames_and_hits(D, [i for i in id_ if i >= 0], "device")
    for f, (x, y) in enumerate(zip(fh, fd)):
        for w, (p, q) in enumerate(zip(x, y)):
            _same(np.asarray(p), np.asarray(q), f"frame / query {f}, buffer {w}")
    H.close(); D.close()


# ---- chunks of 8 (seed 3): three that hold something and one of nothing but Air, the paths of the export the chosen set does not take
SMALL = dict(size=8, chunks_y=8, seed=3)
SMALL_SOLID = [(100, 2, -100), (100, 3, -100), (0, 1, 0)]
SMALL_KEYS = SMALL_SOLID + [(-56, 7, 0)]          # (this world's ground lies in its top chunks: few columns leave cy = 7 empty)
BIG_PAIRS = ALL_PAIRS + [(100 + i, 0) for i in range(280)]          # 304 entries: more than k_grid_encode takes, every grid goes to the host encoder


def _two_frames_and_queries(r, idx, pos):
    r._check(r.L.ycge_scene_update_objects(r.ctx, _prims(idx), len(idx)))
    out = []
    r.SetCamera(pos, 0.0, -1.2)
    for f in range(2):
        r.TryFlipAndBlit(want_sdr=True)
        out.append([r.read(which) for which in FRAME_BUFFERS])
    rng = np.random.default_rng(9)
    o = np.tile(np.asarray(pos, np.float32), (256, 1))
    d = rng.normal(size=(256, 3)).astype(np.float32); d[:, 1] = -np.abs(d[:, 1]) - 0.3
    out.append(list(r.Hit(o, d)) + [r.Occluded(o, d)])
    return out


SMALL_POSE = (WORLD_MIN[0] + 100 * 8 + 4.0, 34.0, WORLD_MIN[2] - 100 * 8 + 4.0)          # just above chunk column (100, -100)


def test_a_lookup_table_too_large_for_the_kernel_takes_the_host_encoder(product_lib):
    """n_lookup > YCGE_ENC_MAX_LOOKUP: the chunks that hold something are made by the host generator and encoded by the host encoder, the
    all-Air one is still made on the device; cells, indices, counters, and frames and queries against an attach of the host's cells."""
    w = _world(**SMALL)
    host = _host_cells(product_lib, w, SMALL_KEYS)
    solid = [bool((c[..., 0] != 0).any()) for c in host]
    assert solid == [True, True, True, False]
    n_solid, n_air = 3, 1
    proto, keep = _proto(BIG_PAIRS)
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    idx, cells = A.GenerateGrids(w, SMALL_KEYS, proto, want_cells=True)
    assert cells.tobytes() == host.tobytes()
    assert idx == [0, 1, 2, -1]
    st, wg = A.grid_pool_stats(), A.worldgen_stats()
    assert st["host_encodes"] == n_solid and st["device_encodes"] == 0 and st["resident"] == n_solid
    assert wg["host_chunks"] == n_solid and wg["device_chunks"] == n_air
    ib = _attach_host(B, product_lib, w, SMALL_SOLID, proto)
    assert ib == idx[:3] and B.grid_pool_stats()["host_encodes"] == n_solid
    fa, fb = _two_frames_and_queries(A, idx[:3], SMALL_POSE), _two_frames_and_queries(B, ib, SMALL_POSE)
    for f, (x, y) in enumerate(zip(fa, fb)):
        for k, (p, q) in enumerate(zip(x, y)):
            _same(np.asarray(p), np.asarray(q), f"frame / query {f}, buffer {k}")
    assert (np.asarray(fa[2][1])[:, 0] >= 0).any() and np.asarray(fa[2][2]).any()          # (the downward rays do meet the chunks)
    A.close(); B.close()


def test_two_devices_give_the_indices_and_frames_of_one(product_lib):
    """A context that drives two devices (both own tiles at 160 x 90): every device gets the columns, the fill and the encode; a peer
    context handed to the export is refused."""
    w = _world(**SMALL)
    proto, keep = _proto(ALL_PAIRS)

    def run(devices):
        r = RaytraceRenderer(_anchor(), 160, 90, devices=devices)
        idx = r.GenerateGrids(w, SMALL_KEYS, proto)
        out = _two_frames_and_queries(r, idx[:3], SMALL_POSE)[:2]
        r.close()
        return idx, out

    (i1, one), (i2, two) = run(None), run([0, 0])
    assert i1 == i2 == [0, 1, 2, -1]
    for f, (x, y) in enumerate(zip(one, two)):
        for k, (p, q) in enumerate(zip(x, y)):
            _same(np.asarray(p), np.asarray(q), f"two devices: frame {f}, buffer {k}")
    r = RaytraceRenderer(_anchor(), 160, 90, devices=[0, 0])
    peer = C.c_void_p(r.L.ycge_debug_peer_context(r.ctx, 0))
    assert peer.value
    before = r.grid_pool_stats()
    karr = np.ascontiguousarray(np.asarray(SMALL_KEYS, np.int32))
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    assert r.L.ycge_scene_generate_grids(peer, C.byref(w), karr.ctypes.data_as(C.POINTER(C.c_int32)), 4, C.byref(proto), out, None) == abi.YCGE_ERR_INVALID_ARG
    assert b"driven by their root" in r.L.ycge_last_error(peer)
    assert list(out) == [-7] * 4 and r.grid_pool_stats() == before
    r.close()


def test_air_chunks_beside_solid_ones_in_two_groups(product_lib):
    """A key list that is mostly Air with want_cells: the Air chunks' cells are made and found empty in launches of their own, the two
    solid chunks fall into two encode groups (YCGE_ENC_GROUP_BYTES below two chunks' raw cells)."""
    w = _world(**SMALL)
    keys = [(-56, 7, 0), (-56, 7, 1), (100, 2, -100), (-55, 7, 2), (-57, 7, 5), (-58, 7, -4), (0, 1, 0), (-55, 7, 5), (-56, 7, -4)]
    host = _host_cells(product_lib, w, keys)
    solid = [bool((c[..., 0] != 0).any()) for c in host]
    assert [k for k, s in zip(keys, solid) if s] == [(100, 2, -100), (0, 1, 0)]
    os.environ["YCGE_ENC_GROUP_BYTES"] = str(8 * 8 * 8 * 8 + 1000)
    try:
        r = RaytraceRenderer(_anchor(), 32, 16)          # (knobs are read when the context is made)
    finally:
        del os.environ["YCGE_ENC_GROUP_BYTES"]
    proto, keep = _proto(ALL_PAIRS)
    idx, cells = r.GenerateGrids(w, keys, proto, want_cells=True)
    assert cells.tobytes() == host.tobytes()
    assert idx == [-1, -1, 0, -1, -1, -1, 1, -1, -1]
    st, wg = r.grid_pool_stats(), r.worldgen_stats()
    assert st["device_encodes"] == 2 and wg["device_chunks"] == len(keys) and wg["host_chunks"] == 0
    r.close()
