"""-m gpu: ycge_scene_generate_world (csrc/ycge_worldgen_scene.cpp over csrc/ycge_worldpregen.hip) against the host generator
(ycge_worldgen_world_cells) - the whole world's cells byte for byte, the indices, and frames and queries bit for bit against a twin
context that attaches the host generator's chunks with ycge_scene_attach_grids.  The windows are tests/test_worldpregen_cpu.py's, which
asserts what they cover and holds the host generator to the restatement."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_worldgen import ALL_PAIRS, FRAME_BUFFERS, _anchor, _prims, _proto, _same
from test_worldpregen_cpu import FOREST4, WINDOWS, host_world
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

pytestmark = pytest.mark.gpu


CASES = dict(WINDOWS, forest4=FOREST4)          # "forest" cut into chunks of 4: all-Air chunks between the ground and a neighbour's canopy


def _world(name):
    S, cy, cx, cz, seed, ox, oz = CASES[name]
    return abi.World(S, cy, seed, abi.Vec3(-cx * S / 2.0, 0.0, -cz * S / 2.0), abi.Vec3(1, 1, 1))          # the window's middle over the world's origin


_HOST = {}


def host_cells(lib, name):
    if name not in _HOST:
        _HOST[name] = host_world(lib, *CASES[name])
    return _HOST[name]


def occupied(cells, S):
    """AttachChunkFromPreloaded's anySolid per chunk, [chunks_x, chunks_y, chunks_z]"""
    nx, ny, nz = cells.shape[:3]
    return (cells[..., 0] != 0).reshape(nx // S, S, ny // S, S, nz // S, S).any(axis=(1, 3, 5))


def expected_indices(cells, S, first=0):
    occ = occupied(cells, S)
    want = np.full(occ.shape, -1, np.int32)
    want[occ] = first + np.arange(int(occ.sum()))          # (cx, cy, cz) order with cx outermost: lowest free first
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_cells_and_indices(product_lib, name):
    S, cy, cx, cz, seed, ox, oz = CASES[name]
    host = host_cells(product_lib, name)
    r = RaytraceRenderer(_anchor(), 32, 16)
    proto, keep = _proto(ALL_PAIRS)
    idx, cells = r.GenerateWorld(_world(name), cx, cz, proto, origin=(ox, oz), want_cells=True)
    assert cells.shape == host.shape and cells.tobytes() == host.tobytes(), int((cells != host).sum())
    want = expected_indices(host, S)
    assert (want == -1).any() and (idx == want).all()          # every window has an all-Air chunk; it takes no slot
    if name == "forest4":          # ... here also UNDER occupied chunks of the same chunk column (tests/test_worldpregen_cpu.py asserts the cells have them)
        occ = want >= 0
        assert (~occ & np.maximum.accumulate(occ[:, ::-1], axis=1)[:, ::-1]).any()
    st, wg, wp = r.grid_pool_stats(), r.worldgen_stats(), r.worldpregen_stats()
    assert st["resident"] == int((want >= 0).sum()) and wg["device_chunks"] == cx * cy * cz and wg["host_chunks"] == 0
    assert wp["any_leaves_passes"] >= (2 if name == "fallback" else 1)          # "fallback" holds a tree with anyLeaves == false: its flag flips in pass 1
    r.close()


def _attach_host(r, world, cells, S, proto):
    """The twin: the chunks that hold something, in (cx, cy, cz) order, through ycge_scene_attach_grids."""
    occ = occupied(cells, S)
    keys = [tuple(int(v) for v in k) for k in np.argwhere(occ)]
    chunks = [np.ascontiguousarray(cells[k[0] * S:(k[0] + 1) * S, k[1] * S:(k[1] + 1) * S, k[2] * S:(k[2] + 1) * S]) for k in keys]
    recs = (abi.Grid * len(keys))()
    wmin = (world.world_min.x, world.world_min.y, world.world_min.z)
    for j, k in enumerate(keys):
        C.memmove(C.byref(recs[j]), C.byref(proto), C.sizeof(abi.Grid))
        recs[j].nx = recs[j].ny = recs[j].nz = S
        recs[j].min_corner = abi.Vec3(*[np.float32(wmin[a]) + np.float32(k[a] * S) * np.float32(1) for a in range(3)])
        recs[j].cells = chunks[j].ctypes.data_as(C.POINTER(C.c_int32))
    out = (C.c_int32 * len(keys))()
    r._check(r.L.ycge_scene_attach_grids(r.ctx, recs, len(keys), out))
    return [int(i) for i in out]


POSE = ((0.5, 118.0, 0.5), 0.3, -1.25)          # above the window's middle, looking down


def _frames_and_queries(r, idx):
    arr = _prims(idx)
    r._check(r.L.ycge_scene_update_objects(r.ctx, arr, len(idx)))
    out = []
    r.SetCamera(*POSE)
    for f in range(2):
        r.TryFlipAndBlit(want_sdr=True)
        out.append([r.read(which) for which in FRAME_BUFFERS])
    rng = np.random.default_rng(9)
    o = np.tile(np.asarray(POSE[0], np.float32), (256, 1))
    d = rng.normal(size=(256, 3)).astype(np.float32); d[:, 1] = -np.abs(d[:, 1]) - 0.3
    out.append(list(r.Hit(o, d)) + [r.Occluded(o, d)])
    return out


def _all_same(a, b, label):
    for f, (x, y) in enumerate(zip(a, b)):
        for w, (p, q) in enumerate(zip(x, y)):
            _same(np.asarray(p), np.asarray(q), f"{label}: frame / query {f}, buffer {w}")


@pytest.mark.parametrize("in_flight", [0, 2])
def test_frames_and_queries_equal_an_attach_of_the_host_cells(product_lib, in_flight):
    name = "forest"
    S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
    world, host = _world(name), host_cells(product_lib, name)
    proto, keep = _proto(ALL_PAIRS)
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    for r in (A, B):
        r.SetCamera(*POSE)
        for _ in range(in_flight):
            r.RenderAsync()
    ia = [int(i) for i in A.GenerateWorld(world, cx, cz, proto, origin=(ox, oz)).ravel() if i >= 0]
    ib = _attach_host(B, world, host, S, proto)
    assert ia == ib
    fa, fb = _frames_and_queries(A, ia), _frames_and_queries(B, ib)
    _all_same(fa, fb, "generated against attached")
    assert (np.asarray(fa[2][1])[:, 0] >= 0).any() and np.asarray(fa[2][2]).any()          # (the downward rays do meet the chunks)
    A.close(); B.close()


def test_sub_batches_of_one_chunk_give_the_same_cells(product_lib):
    """YCGE_ENC_GROUP_BYTES below two chunks' raw cells: every fill launch holds ONE chunk, so a canopy that crosses a chunk border is made in
    another sub-batch than its root (the window has such trees in x, y and z)."""
    name = "forest"
    S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
    host = host_cells(product_lib, name)
    os.environ["YCGE_ENC_GROUP_BYTES"] = str(S * S * S * 8 + 1000)
    try:
        r = RaytraceRenderer(_anchor(), 32, 16)          # (knobs are read when the context is made)
    finally:
        del os.environ["YCGE_ENC_GROUP_BYTES"]
    proto, keep = _proto(ALL_PAIRS)
    idx, cells = r.GenerateWorld(_world(name), cx, cz, proto, origin=(ox, oz), want_cells=True)
    assert cells.tobytes() == host.tobytes() and (idx == expected_indices(host, S)).all()
    r.close()


def _replay(r, idx):
    """the same frames and queries from the same start: frame counter 0, the TAA history dropped (ycge_resize does), the same pose"""
    r._check(r.L.ycge_resize(r.ctx, r.fbW, r.fbH, r.ss))
    r._check(r.L.ycge_set_frame_counter(r.ctx, 0))
    return _frames_and_queries(r, idx)


def test_a_refused_call_leaves_the_frames_as_they_were(product_lib):
    L = product_lib
    S, cy, cx, cz, seed, ox, oz = WINDOWS["small"]
    world = _world("small")
    proto, keep = _proto(ALL_PAIRS)
    r = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    idx = [int(i) for i in r.GenerateWorld(world, cx, cz, proto, origin=(ox, oz)).ravel() if i >= 0]
    before, pool = _replay(r, idx), r.grid_pool_stats()
    n = cx * cy * cz
    out = np.full(n, -7, np.int32)
    po = out.ctypes.data_as(C.POINTER(C.c_int32))

    def unchanged(label):
        assert (out == -7).all(), label
        st = r.grid_pool_stats()
        assert (st["resident"], st["arena_in_use"], st["free_indices"]) == (pool["resident"], pool["arena_in_use"], pool["free_indices"]), label
        _all_same(before, _replay(r, idx), label)

    few, keep2 = _proto([p for p in ALL_PAIRS if p != (1, 1)], default_material=-1)          # no (Stone, 1): rock piles and strata write it
    for flight in (0, 2):
        if flight:
            r._check(L.ycge_resize(r.ctx, r.fbW, r.fbH, r.ss)); r._check(L.ycge_set_frame_counter(r.ctx, 0))
            r.SetCamera(*POSE)
        for _ in range(flight):
            r.RenderAsync()
        assert L.ycge_scene_generate_world(r.ctx, C.byref(world), cx, cz, ox, oz, C.byref(few), po, None) == abi.YCGE_ERR_INVALID_ARG
        assert b"no material" in L.ycge_last_error(r.ctx) and b"metaId 1" in L.ycge_last_error(r.ctx)
        r.Wait()
        unchanged(f"a lookup without (Stone, 1), {flight} frames in flight")
    # the argument refusals, none of which touches cells_out
    cells = np.full((cx * S, cy * S, cz * S, 2), -9, np.int32)
    pc = cells.ctypes.data_as(C.POINTER(C.c_int32))
    lim = 1 << 24
    bad_world = abi.World(3, cy, seed, world.world_min, world.voxel_size)
    for w, a, b, x, z in ((bad_world, cx, cz, ox, oz), (world, 0, cz, ox, oz), (world, cx, 0, ox, oz), (world, cx, cz, lim, oz), (world, cx, cz, ox, -lim - 1)):
        assert L.ycge_scene_generate_world(r.ctx, C.byref(w), a, b, x, z, C.byref(proto), po, pc) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_scene_generate_world(r.ctx, C.byref(abi.World(64, 16, 0, world.world_min, world.voxel_size)), 16, 16, 0, 0, C.byref(proto), po, pc) == abi.YCGE_ERR_INVALID_ARG
    empty = RaytraceRenderer(None, 32, 16)
    assert L.ycge_scene_generate_world(empty.ctx, C.byref(world), cx, cz, ox, oz, C.byref(proto), po, pc) == abi.YCGE_ERR_NO_SCENE
    empty.close()
    assert (cells == -9).all()
    unchanged("argument refusals")
    # a later call takes the next indices
    again = r.GenerateWorld(world, cx, cz, proto, origin=(ox, oz))
    assert sorted(int(i) for i in again.ravel() if i >= 0) == list(range(len(idx), 2 * len(idx)))
    r.close()


def test_the_host_knob_gives_the_same_cells_and_frames(product_lib):
    name = "forest"
    S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
    world, host = _world(name), host_cells(product_lib, name)
    proto, keep = _proto(ALL_PAIRS)
    os.environ["YCGE_WORLDGEN_HOST"] = "1"
    try:
        H = RaytraceRenderer(_anchor(), 96, 27, 60.0)          # (knobs are read when the context is made)
    finally:
        del os.environ["YCGE_WORLDGEN_HOST"]
    D = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    ih, ch = H.GenerateWorld(world, cx, cz, proto, origin=(ox, oz), want_cells=True)
    id_, cd = D.GenerateWorld(world, cx, cz, proto, origin=(ox, oz), want_cells=True)
    assert (ih == id_).all() and ch.tobytes() == cd.tobytes() == host.tobytes()
    n = cx * cy * cz
    assert H.worldgen_stats()["host_chunks"] == n and H.worldgen_stats()["device_chunks"] == 0 and D.worldgen_stats()["device_chunks"] == n
    fh = _frames_and_queries(H, [int(i) for i in ih.ravel() if i >= 0])
    fd = _frames_and_queries(D, [int(i) for i in id_.ravel() if i >= 0])
    _all_same(fh, fd, "host knob against device")
    H.close(); D.close()


def test_a_lookup_table_too_large_for_the_kernel_takes_the_host_world(product_lib):
    """n_lookup > YCGE_ENC_MAX_LOOKUP: the whole world is made by the host generator and every occupied chunk goes through the host
    encoder; cells, indices, counters, and frames and queries against an attach of the host's chunks."""
    name = "small"
    S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
    world, host = _world(name), host_cells(product_lib, name)
    proto, keep = _proto(ALL_PAIRS + [(100 + i, 0) for i in range(280)])
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    idx, cells = A.GenerateWorld(world, cx, cz, proto, origin=(ox, oz), want_cells=True)
    assert cells.shape == host.shape and cells.tobytes() == host.tobytes()
    want = expected_indices(host, S)
    assert (idx == want).all()
    n_occ = int((want >= 0).sum())
    st, wg = A.grid_pool_stats(), A.worldgen_stats()
    assert st["host_encodes"] == n_occ and st["device_encodes"] == 0 and st["resident"] == n_occ
    assert wg["host_chunks"] == cx * cy * cz and wg["device_chunks"] == 0
    ia = [int(i) for i in idx.ravel() if i >= 0]
    ib = _attach_host(B, world, host, S, proto)
    assert ia == ib
    fa, fb = _frames_and_queries(A, ia), _frames_and_queries(B, ib)
    _all_same(fa, fb, "generated against attached")
    assert (np.asarray(fa[2][1])[:, 0] >= 0).any() and np.asarray(fa[2][2]).any()          # (the downward rays do meet the chunks)
    A.close(); B.close()


def test_two_devices_give_the_indices_and_frames_of_one(product_lib):
    """A context that drives two devices (both own tiles at 160 x 90) on the window whose anyLeaves passes number two at least: the peer
    repeats the root's passes without reading anything back.  A peer context handed to the export is refused."""
    name = "fallback"
    S, cy, cx, cz, seed, ox, oz = WINDOWS[name]
    world = _world(name)
    proto, keep = _proto(ALL_PAIRS)

    def run(devices):
        r = RaytraceRenderer(_anchor(), 160, 90, devices=devices)
        idx = r.GenerateWorld(world, cx, cz, proto, origin=(ox, oz))
        assert r.worldpregen_stats()["any_leaves_passes"] >= 2
        out = _frames_and_queries(r, [int(i) for i in idx.ravel() if i >= 0])[:2]
        r.close()
        return idx, out

    (i1, one), (i2, two) = run(None), run([0, 0])
    assert (i1 == i2).all() and (i1 == expected_indices(host_cells(product_lib, name), S)).all()
    _all_same(one, two, "two devices against one")
    r = RaytraceRenderer(_anchor(), 160, 90, devices=[0, 0])
    peer = C.c_void_p(r.L.ycge_debug_peer_context(r.ctx, 0))
    assert peer.value
    before = r.grid_pool_stats()
    out = np.full(cx * cy * cz, -7, np.int32)
    assert r.L.ycge_scene_generate_world(peer, C.byref(world), cx, cz, ox, oz, C.byref(proto), out.ctypes.data_as(C.POINTER(C.c_int32)), None) == abi.YCGE_ERR_INVALID_ARG
    assert b"driven by their root" in r.L.ycge_last_error(peer)
    assert (out == -7).all() and r.grid_pool_stats() == before
    r.close()
