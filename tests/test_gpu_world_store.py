"""-m gpu: the world store (csrc/ycge_world_store.cpp over csrc/ycge_world_store.hip) against the host path the project already trusts -
world_file.slice_chunk and ycge_scene_attach_grids.  Occupancy and raw slices byte for byte; indices, read_grid records and materials,
frames and queries bit for bit against a twin context that attaches the host's slices.  The worlds are tests/test_world_store_cpu.py's,
which asserts what they cover."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_worldgen import ALL_PAIRS, FRAME_BUFFERS, _anchor, _prims, _proto, _same
from test_gpu_worldpregen import _all_same, expected_indices
from test_world_store_cpu import INSIDE_KINDS, SPECS, WORLDS, all_keys, chunk_slices, counts, occupied
from test_worldpregen_cpu import WINDOWS, host_world
from yetanotherconsolegameengine_amd import abi, world_file as wf
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

pytestmark = pytest.mark.gpu

WORLD_MIN = (-10.0, 0.0, -9.0)
POSE = ((0.5, 30.0, 0.5), 0.3, -1.25)          # above the tiny worlds, looking down
I32P = C.POINTER(C.c_int32)


def _with_env(env, make):
    """a renderer made with these knobs set (they are read when the context is made)"""
    before = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return make()
    finally:
        for k, v in before.items():          # (a value set from outside the suite comes back)
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _store_proto(pairs=ALL_PAIRS, default_material=-1, world_min=WORLD_MIN):
    proto, keep = _proto(pairs, default_material)
    proto.min_corner = abi.Vec3(*world_min)
    return proto, keep


def _attach_host(r, cells, S, keys, proto):
    """The twin: slice_chunk's cells of the keys that hold anything, in the same order, through ycge_scene_attach_grids -> index per key (-1: none)."""
    parts = [(j, wf.slice_chunk(cells, *k, S)) for j, k in enumerate(keys)]
    parts = [(j, p) for j, p in parts if p is not None]
    recs = (abi.Grid * max(1, len(parts)))()
    wmin = (proto.min_corner.x, proto.min_corner.y, proto.min_corner.z)
    for n, (j, p) in enumerate(parts):
        C.memmove(C.byref(recs[n]), C.byref(proto), C.sizeof(abi.Grid))
        recs[n].nx, recs[n].ny, recs[n].nz = p.shape[:3]
        recs[n].min_corner = abi.Vec3(*[np.float32(wmin[a]) + np.float32(keys[j][a] * S) * np.float32(1) for a in range(3)])
        recs[n].cells = p.ctypes.data_as(I32P)
    out = (C.c_int32 * max(1, len(parts)))()
    r._check(r.L.ycge_scene_attach_grids(r.ctx, recs, len(parts), out))
    idx = [-1] * len(keys)
    for n, (j, p) in enumerate(parts):
        idx[j] = int(out[n])
    return idx


def _frames_and_queries(r, idx, pose=POSE):
    arr = _prims(idx)
    r._check(r.L.ycge_scene_update_objects(r.ctx, arr, len(idx)))
    out = []
    r.SetCamera(*pose)
    for f in range(2):
        r.TryFlipAndBlit(want_sdr=True)
        out.append([r.read(which) for which in FRAME_BUFFERS])
    rng = np.random.default_rng(9)
    o = np.tile(np.asarray(pose[0], np.float32), (256, 1))
    d = rng.normal(size=(256, 3)).astype(np.float32); d[:, 1] = -np.abs(d[:, 1]) - 0.3
    out.append(list(r.Hit(o, d)) + [r.Occluded(o, d)])
    return out


def _replay(r, idx, pose=POSE):
    """the same frames and queries from the same start: frame counter 0, the TAA history dropped (ycge_resize does), the same pose"""
    r._check(r.L.ycge_resize(r.ctx, r.fbW, r.fbH, r.ss))
    r._check(r.L.ycge_set_frame_counter(r.ctx, 0))
    return _frames_and_queries(r, idx, pose)


def _grids_same(A, ia, B, ib, cells, S, keys, label):
    for k, a, b in zip(keys, ia, ib):
        assert (a >= 0) == (b >= 0), (label, k)
        if a < 0:
            continue
        shape = cells[chunk_slices(cells.shape[:3], S, k)].shape[:3]
        (ra, ma), (rb, mb) = A.read_grid(a, shape), B.read_grid(b, shape)
        assert ra.tobytes() == rb.tobytes() and ma.tobytes() == mb.tobytes(), (label, k)


def _live(lib):
    out = (C.c_int64 * 6)()
    assert lib.ycge_debug_live_resources(out) == abi.YCGE_OK
    return [int(v) for v in out]


def _mixed_keys(name):
    """every chunk, nearest the far corner first, then: one named again, a negative one, two beyond the counts (the all-air chunk is among the first)"""
    n = counts(*SPECS[name])
    keys = sorted(all_keys(name), key=lambda k: ((k[0] - n[0] + 1) ** 2 + (k[2] - n[2] + 1) ** 2, k[1]))
    return keys + [keys[0], (-1, 0, 0), (n[0], 0, 0), (0, n[1] + 3, 0), (0, 0, 0)]


# ---------------------------------------------------------------- 1. occupancy and slices
ALL_WORLDS = dict(WORLDS, **{f"inside_{k}": v for k, v in INSIDE_KINDS.items()})


@pytest.mark.parametrize("mode", ["one_slab", "plane_slabs", "four_plane_slabs", "page_locked"])
@pytest.mark.parametrize("name", list(ALL_WORLDS))
def test_occupancy_and_slices(product_lib, name, mode):
    cells = ALL_WORLDS[name]
    dims, S = SPECS[name.split("_")[0] if name.startswith("inside") else name]
    # a slab = one x-plane: slab borders inside chunks; four planes (and a few bytes: whole planes only): the last slab is a partial one (11 = 4 + 4 + 3, 21 = 5 x 4 + 1)
    per = {"plane_slabs": 1, "four_plane_slabs": min(4, dims[0])}.get(mode)
    env = {"YCGE_WORLD_STORE_SLAB_BYTES": per * dims[1] * dims[2] * 8 + (7 if per > 1 else 0)} if per else {}
    r = _with_env(env, lambda: RaytraceRenderer(None, 32, 16))
    src = cells
    if mode == "page_locked":
        src, owner = r._page_locked_zeros(cells.shape, np.int32)
        src[...] = cells
    assert r.LoadWorld(src, S) == dims
    got_dims, got_S, occ = r.WorldInfo()
    assert got_dims == dims and got_S == S
    assert occ.tobytes() == occupied(cells, S).tobytes(), (occ, occupied(cells, S))
    st = r.world_store_stats()
    assert st["store_bytes"] == cells.nbytes and st["slabs"] == (-(-dims[0] // per) if per else 1)
    if mode == "page_locked":
        assert st["load_stage_us"] == 0
    for key in np.ndindex(*occ.shape):
        want = np.ascontiguousarray(cells[chunk_slices(dims, S, key)])
        got = r.world_store_chunk(*key)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (name, key)
    r.close()


def test_a_world_file_is_loaded_from_its_path(product_lib, tmp_path):
    cells, (dims, S) = WORLDS["clip"], SPECS["clip"]
    wf.write_vg01(tmp_path / "w.vg", cells)
    r = RaytraceRenderer(None, 32, 16)
    assert r.LoadWorld(tmp_path / "w.vg", S) == dims
    assert r.WorldInfo()[2].tobytes() == occupied(cells, S).tobytes()
    assert r.world_store_chunk(2, 1, 2).tobytes() == np.ascontiguousarray(cells[chunk_slices(dims, S, (2, 1, 2))]).tobytes()
    (tmp_path / "bad.vg").write_bytes(b"VG02" + (tmp_path / "w.vg").read_bytes()[4:])
    with pytest.raises(abi.YcgeError, match="Expected 'VG01'"):
        r.LoadWorld(tmp_path / "bad.vg", S)
    assert r.WorldInfo()[0] == dims
    r.close()


# ---------------------------------------------------------------- 2. attach equals an attach of the host slices
@pytest.mark.parametrize("in_flight", [0, 2])
@pytest.mark.parametrize("name", ["clip", "odd"])
def test_attach_equals_an_attach_of_the_host_slices(product_lib, name, in_flight):
    cells, (dims, S) = WORLDS[name], SPECS[name]
    keys = _mixed_keys(name)
    proto, keep = _store_proto()
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    A.LoadWorld(cells, S)
    for r in (A, B):
        r.SetCamera(*POSE)
        for _ in range(in_flight):
            r.RenderAsync()
    ia = A.AttachWorldChunks(keys, proto)
    ib = _attach_host(B, cells, S, keys, proto)
    occ = occupied(cells, S)
    n_all = len(all_keys(name))
    assert ia == ib
    assert [i >= 0 for i in ia[:n_all]] == [bool(occ[k]) for k in keys[:n_all]] and ia[n_all] >= 0 and ia[n_all] != ia[0] and ia[n_all + 1:] == [-1] * 4
    assert sorted(i for i in ia if i >= 0) == list(range(int(occ.sum()) + 1))          # lowest free first, one more for the key named twice
    assert A.world_store_stats()["device_chunks"] == int(occ.sum()) + 1 and A.world_store_stats()["host_chunks"] == 0
    _grids_same(A, ia, B, ib, cells, S, keys, name)
    fa, fb = _frames_and_queries(A, [i for i in ia if i >= 0]), _frames_and_queries(B, [i for i in ib if i >= 0])
    _all_same(fa, fb, "attached by key against attached host slices")
    assert (np.asarray(fa[2][1])[:, 0] >= 0).any() and np.asarray(fa[2][2]).any()          # (the downward rays do meet the chunks)
    A.close(); B.close()


# ---------------------------------------------------------------- 3. sub-batches
def test_sub_batches_of_one_chunk_give_the_same_grids(product_lib):
    name = "clip"
    cells, (dims, S) = WORLDS[name], SPECS[name]
    keys = _mixed_keys(name)
    proto, keep = _store_proto()
    A = _with_env({"YCGE_ENC_GROUP_BYTES": S * S * S * 8 + 1000}, lambda: RaytraceRenderer(_anchor(), 32, 16))          # below two chunks' raw cells
    B = RaytraceRenderer(_anchor(), 32, 16)
    A.LoadWorld(cells, S); B.LoadWorld(cells, S)
    ia, ib = A.AttachWorldChunks(keys, proto), B.AttachWorldChunks(keys, proto)
    assert ia == ib == _attach_host(RaytraceRenderer(_anchor(), 32, 16), cells, S, keys, proto)
    _grids_same(A, ia, B, ib, cells, S, keys, "sub-batches")
    A.close(); B.close()


# ---------------------------------------------------------------- 4. a generated world round-trips
def test_a_generated_world_round_trips(product_lib):
    import test_gpu_worldpregen as wp
    S, cy, cx, cz, seed, ox, oz = WINDOWS["small"]
    cells = host_world(product_lib, *WINDOWS["small"])          # ycge_worldgen_world_cells: the VG01 payload
    world = wp._world("small")
    proto, keep = _store_proto(world_min=(world.world_min.x, world.world_min.y, world.world_min.z))
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    A.LoadWorld(cells, S)
    keys = [(x, y, z) for x in range(cx) for y in range(cy) for z in range(cz)]
    ia = np.asarray(A.AttachWorldChunks(keys, proto), np.int32).reshape(cx, cy, cz)
    want = expected_indices(cells, S)
    assert (want == -1).any() and (ia == want).all()
    ib = B.GenerateWorld(world, cx, cz, proto, origin=(ox, oz))
    assert (ib == want).all()
    fa = _frames_and_queries(A, [int(i) for i in ia.ravel() if i >= 0], wp.POSE)
    fb = _frames_and_queries(B, [int(i) for i in ib.ravel() if i >= 0], wp.POSE)
    _all_same(fa, fb, "loaded and attached against generated")
    assert (np.asarray(fa[2][1])[:, 0] >= 0).any() and np.asarray(fa[2][2]).any()
    A.close(); B.close()


# ---------------------------------------------------------------- 5. refusals leave everything as it was
def test_refusals_leave_everything_as_it_was(product_lib):
    L = product_lib
    name = "clip"
    cells, (dims, S) = WORLDS[name], SPECS[name]
    keys = all_keys(name)
    proto, keep = _store_proto()
    r = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    out = np.full(len(keys), -7, np.int32)
    po = out.ctypes.data_as(I32P)
    karr = np.ascontiguousarray(np.asarray(keys, np.int32))
    pk = karr.ctypes.data_as(I32P)
    # no store
    assert L.ycge_scene_attach_world_chunks(r.ctx, pk, len(keys), C.byref(proto), po) == abi.YCGE_ERR_INVALID_ARG
    assert b"no world store" in L.ycge_last_error(r.ctx)
    assert L.ycge_world_store_info(r.ctx, None, None, None, 0) == abi.YCGE_ERR_INVALID_ARG and b"no world store" in L.ycge_last_error(r.ctx)
    assert L.ycge_world_store_release(r.ctx) == abi.YCGE_OK
    assert (out == -7).all()
    r.LoadWorld(cells, S)
    idx = [i for i in r.AttachWorldChunks(keys, proto) if i >= 0]
    before, pool, info = _replay(r, idx), r.grid_pool_stats(), r.WorldInfo()

    def unchanged(label, store=True):
        assert (out == -7).all(), label
        st = r.grid_pool_stats()
        assert (st["resident"], st["arena_in_use"], st["free_indices"]) == (pool["resident"], pool["arena_in_use"], pool["free_indices"]), label
        if store:
            now = r.WorldInfo()
            assert now[:2] == info[:2] and now[2].tobytes() == info[2].tobytes(), label
        _all_same(before, _replay(r, idx), label)

    # no store, with grids resident and frames to compare: the store released, the refusal, the store loaded again
    r.ReleaseWorld()
    assert L.ycge_scene_attach_world_chunks(r.ctx, pk, len(keys), C.byref(proto), po) == abi.YCGE_ERR_INVALID_ARG
    assert b"no world store" in L.ycge_last_error(r.ctx)
    unchanged("no store", store=False)
    r.LoadWorld(cells, S)

    # a lookup without (2, 1) and no default material: named by chunk key and cell, the first such chunk in the call's order and its lowest cell
    few, keep2 = _store_proto([p for p in ALL_PAIRS if p != (2, 1)], default_material=-1)
    first = next(k for k in keys if wf.slice_chunk(cells, *k, S) is not None and ((wf.slice_chunk(cells, *k, S) == (2, 1)).all(axis=-1)).any())
    part = wf.slice_chunk(cells, *first, S)
    cell = np.unravel_index(int(np.flatnonzero((part == (2, 1)).all(axis=-1).ravel())[0]), part.shape[:3])
    for flight in (0, 2):
        if flight:
            r._check(L.ycge_resize(r.ctx, r.fbW, r.fbH, r.ss)); r._check(L.ycge_set_frame_counter(r.ctx, 0))
            r.SetCamera(*POSE)
        for _ in range(flight):
            r.RenderAsync()
        assert L.ycge_scene_attach_world_chunks(r.ctx, pk, len(keys), C.byref(few), po) == abi.YCGE_ERR_INVALID_ARG
        msg = L.ycge_last_error(r.ctx).decode()
        assert "no material for (matId 2, metaId 1)" in msg and "chunk (%d, %d, %d)" % first in msg and "cell (%d, %d, %d)" % tuple(int(v) for v in cell) in msg, msg
        r.Wait()
        unchanged(f"a lookup without (2, 1), {flight} frames in flight")
    # argument refusals
    assert L.ycge_scene_attach_world_chunks(r.ctx, None, 3, C.byref(proto), po) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_scene_attach_world_chunks(r.ctx, pk, -1, C.byref(proto), po) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_scene_attach_world_chunks(r.ctx, pk, len(keys), None, po) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_scene_attach_world_chunks(r.ctx, pk, len(keys), C.byref(proto), None) == abi.YCGE_ERR_INVALID_ARG
    # a failed load leaves the store that was there
    pc = cells.ctypes.data
    for nx, ny, nz, cs in ((0, 13, 19, S), (21, -1, 19, S), (21, 13, 19, 0), (21, 13, 19, 1025), (1024, 1024, 1024, 32), (21, 13, 19, -4)):
        assert L.ycge_world_store_load(r.ctx, pc, nx, ny, nz, cs) == abi.YCGE_ERR_INVALID_ARG, (nx, ny, nz, cs)
    assert L.ycge_world_store_load(r.ctx, None, 21, 13, 19, S) == abi.YCGE_ERR_INVALID_ARG
    assert L.ycge_world_store_info(r.ctx, None, None, out.ctypes.data, 3) == abi.YCGE_ERR_INVALID_ARG          # room for 3 of 18 chunks
    unchanged("argument refusals and failed loads")
    # no scene
    empty = RaytraceRenderer(None, 32, 16)
    empty.LoadWorld(cells, S)
    assert L.ycge_scene_attach_world_chunks(empty.ctx, pk, len(keys), C.byref(proto), po) == abi.YCGE_ERR_NO_SCENE
    empty.close()
    unchanged("no scene")
    # a later attach takes the next indices
    again = [i for i in r.AttachWorldChunks(keys, proto) if i >= 0]
    assert again == list(range(len(idx), 2 * len(idx)))
    r.close()


# ---------------------------------------------------------------- 6. replace and release
def test_replace_and_release(product_lib):
    L = product_lib
    start = _live(L)
    proto, keep = _store_proto()
    r = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    r.TryFlipAndBlit(want_sdr=True)
    r.Hit(np.zeros((1, 3), np.float32), np.asarray([[0, -1, 0]], np.float32))          # (what the frames and queries allocate is there before the store)
    c1, (d1, S1) = WORLDS["clip"], SPECS["clip"]
    c2, (d2, S2) = WORLDS["odd"], SPECS["odd"]
    held = _live(L)
    r.LoadWorld(c1, S1)
    with_store = _live(L)
    assert with_store[0] == held[0] + 1 and with_store[1] - held[1] >= c1.nbytes == r.world_store_stats()["store_bytes"]
    assert with_store[2:] == held[2:]          # the load's streams, events and staging are gone with it
    idx = [i for i in r.AttachWorldChunks(all_keys("clip"), proto) if i >= 0]
    first = _replay(r, idx)
    r.LoadWorld(c2, S2)          # replaces the store; the grids are encoded copies
    info = r.WorldInfo()
    assert info[0] == d2 and info[1] == S2 and info[2].tobytes() == occupied(c2, S2).tobytes()
    _all_same(first, _replay(r, idx), "after a second world was loaded")
    more = [i for i in r.AttachWorldChunks(all_keys("odd"), proto) if i >= 0]
    assert more == list(range(len(idx), len(idx) + int(occupied(c2, S2).sum())))
    r._check(L.ycge_scene_upload(r.ctx, r.flat.byref()))          # the store is not scene state
    assert r.WorldInfo()[0] == d2
    idx = [i for i in r.AttachWorldChunks(all_keys("odd"), proto) if i >= 0]
    first = _replay(r, idx)
    before_release = _live(L)
    r.ReleaseWorld()
    after = _live(L)
    assert after[0] == before_release[0] - 1 and before_release[1] - after[1] >= c2.nbytes and r.world_store_stats()["store_bytes"] == 0
    with pytest.raises(abi.YcgeError, match="no world store"):
        r.WorldInfo()
    _all_same(first, _replay(r, idx), "after the store was released")
    r.LoadWorld(c1, S1)          # ycge_destroy releases a store too
    r.close()
    assert _live(L) == start


# ---------------------------------------------------------------- 7. the host knob and a large lookup table
def test_the_host_knob_gives_the_same_grids_and_frames(product_lib):
    name = "clip"
    cells, (dims, S) = WORLDS[name], SPECS[name]
    keys = _mixed_keys(name)
    proto, keep = _store_proto()
    H = _with_env({"YCGE_WORLD_STORE_HOST": 1}, lambda: RaytraceRenderer(_anchor(), 96, 27, 60.0))
    D = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    H.LoadWorld(cells, S); D.LoadWorld(cells, S)
    assert H.WorldInfo()[2].tobytes() == D.WorldInfo()[2].tobytes() == occupied(cells, S).tobytes()
    for key in all_keys(name):
        assert H.world_store_chunk(*key).tobytes() == D.world_store_chunk(*key).tobytes()
    ih, id_ = H.AttachWorldChunks(keys, proto), D.AttachWorldChunks(keys, proto)
    assert ih == id_
    n = sum(i >= 0 for i in ih)
    sh, sd = H.world_store_stats(), D.world_store_stats()
    assert (sh["host_chunks"], sh["device_chunks"], sd["host_chunks"], sd["device_chunks"]) == (n, 0, 0, n)
    _grids_same(H, ih, D, id_, cells, S, keys, "host knob")
    _all_same(_frames_and_queries(H, [i for i in ih if i >= 0]), _frames_and_queries(D, [i for i in id_ if i >= 0]), "host knob against device")
    H.close(); D.close()


def test_a_lookup_table_too_large_for_the_kernel_takes_the_host_encoder(product_lib):
    """n_lookup > YCGE_ENC_MAX_LOOKUP: every chunk's rows are copied out of the device store for the host encoder."""
    name = "odd"
    cells, (dims, S) = WORLDS[name], SPECS[name]
    keys = _mixed_keys(name)
    proto, keep = _store_proto(ALL_PAIRS + [(100 + i, 0) for i in range(280)])
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    A.LoadWorld(cells, S)
    ia, ib = A.AttachWorldChunks(keys, proto), _attach_host(B, cells, S, keys, proto)
    assert ia == ib
    n = sum(i >= 0 for i in ia)
    st, ws = A.grid_pool_stats(), A.world_store_stats()
    assert st["host_encodes"] == n and st["device_encodes"] == 0 and ws["host_chunks"] == n and ws["device_chunks"] == 0
    _grids_same(A, ia, B, ib, cells, S, keys, "large lookup")
    _all_same(_frames_and_queries(A, [i for i in ia if i >= 0]), _frames_and_queries(B, [i for i in ib if i >= 0]), "large lookup against attached")
    A.close(); B.close()


# ---------------------------------------------------------------- 8. two devices
def test_two_devices_give_the_indices_and_frames_of_one(product_lib):
    name = "clip"
    cells, (dims, S) = WORLDS[name], SPECS[name]
    keys = _mixed_keys(name)
    proto, keep = _store_proto()

    def run(devices):
        r = RaytraceRenderer(_anchor(), 160, 90, devices=devices)
        r.LoadWorld(cells, S)
        idx = r.AttachWorldChunks(keys, proto)
        out = _frames_and_queries(r, [i for i in idx if i >= 0])[:2]
        r.close()
        return idx, out

    (i1, one), (i2, two) = run(None), run([0, 0])
    assert i1 == i2
    _all_same(one, two, "two devices against one")
    r = RaytraceRenderer(_anchor(), 160, 90, devices=[0, 0])
    r.LoadWorld(cells, S)
    L = r.L
    peer = C.c_void_p(L.ycge_debug_peer_context(r.ctx, 0))
    assert peer.value
    resident = [i for i in r.AttachWorldChunks(keys, proto) if i >= 0]
    frames = _replay(r, resident)
    before, info = r.grid_pool_stats(), r.WorldInfo()
    out = np.full(len(keys), -7, np.int32)
    karr = np.ascontiguousarray(np.asarray(keys, np.int32))
    calls = (lambda: L.ycge_scene_attach_world_chunks(peer, karr.ctypes.data_as(I32P), len(keys), C.byref(proto), out.ctypes.data_as(I32P)),
             lambda: L.ycge_world_store_load(peer, cells.ctypes.data, *dims, S),
             lambda: L.ycge_world_store_info(peer, None, None, None, 0),
             lambda: L.ycge_world_store_release(peer))
    for call in calls:
        assert call() == abi.YCGE_ERR_INVALID_ARG
        assert b"driven by their root" in L.ycge_last_error(peer)
    now = r.WorldInfo()
    assert (out == -7).all() and r.grid_pool_stats() == before and now[:2] == info[:2] and now[2].tobytes() == info[2].tobytes()
    _all_same(frames, _replay(r, resident), "after the peer was refused")
    r.close()


# ---------------------------------------------------------------- 9. the attach's limit of 255 distinct pairs holds for a file's cells
def _pairs_world():
    """16 x 8 x 8, chunks of 8: chunk (0, 0, 0) holds 255 distinct solid pairs, chunk (1, 0, 0) holds 300 - most of them miss the lookup"""
    cells = np.zeros((16, 8, 8, 2), np.int32)
    for cx, n in ((0, 255), (1, 300)):
        i = np.arange(512) % n
        part = np.stack([1 + i % 20, i // 20], axis=-1).astype(np.int32).reshape(8, 8, 8, 2)
        cells[cx * 8:(cx + 1) * 8] = part
    return cells


@pytest.mark.parametrize("knob", ["device", "host", "large_lookup"])
def test_more_than_255_distinct_pairs_are_refused_as_the_attach_refuses_them(product_lib, knob):
    L = product_lib
    cells, S = _pairs_world(), 8
    assert len({tuple(p) for p in cells[:8].reshape(-1, 2)}) == 255 and len({tuple(p) for p in cells[8:].reshape(-1, 2)}) == 300
    pairs = ALL_PAIRS + ([(100 + i, 0) for i in range(280)] if knob == "large_lookup" else [])
    proto, keep = _store_proto(pairs, default_material=0)          # a default material: a lookup miss alone is no refusal
    A = _with_env({"YCGE_WORLD_STORE_HOST": 1} if knob == "host" else {}, lambda: RaytraceRenderer(_anchor(), 96, 27, 60.0))
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    A.LoadWorld(cells, S)
    ok = [(0, 0, 0)]
    ia, ib = A.AttachWorldChunks(ok, proto), _attach_host(B, cells, S, ok, proto)
    assert ia == ib == [0]
    _grids_same(A, ia, B, ib, cells, S, ok, "255 pairs")
    before, pool = _replay(A, ia), A.grid_pool_stats()
    both = [(0, 0, 0), (1, 0, 0)]
    with pytest.raises(abi.YcgeError) as ea:
        A.AttachWorldChunks(both, proto)
    with pytest.raises(abi.YcgeError) as eb:
        _attach_host(B, cells, S, both, proto)
    assert ea.value.status == eb.value.status == abi.YCGE_ERR_UNSUPPORTED
    assert "more than 255 distinct" in str(ea.value) and "more than 255 distinct" in str(eb.value) and "chunk (1, 0, 0)" in str(ea.value), str(ea.value)
    st = A.grid_pool_stats()
    assert (st["resident"], st["arena_in_use"], st["free_indices"]) == (pool["resident"], pool["arena_in_use"], pool["free_indices"])
    _all_same(before, _replay(A, ia), "after the refusal")
    assert A.AttachWorldChunks(ok, proto) == _attach_host(B, cells, S, ok, proto) == [1]
    A.close(); B.close()
