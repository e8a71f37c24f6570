"""-m gpu: a world store whose source is the generator (ycge_world_store_generate, both forms), its planes read back (ycge_world_store_read)
and its chunks attached by key, against the host generator ycge_worldgen_world_cells - held to tests/worldpregen_restatement.py by
tests/test_worldpregen_cpu.py - and, for attaches, a twin context that does ycge_world_store_load of those cells.  Everything byte for
byte and bit for bit; no tolerance anywhere.  The windows are test_worldpregen_cpu.WINDOWS plus FOREST4, which that file asserts to hold
canopies across chunk borders in x, y and z, a tree with anyLeaves == false, the ocean edge, the reference's own origin and all-Air chunks
under occupied ones."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_worldgen import ALL_PAIRS, _anchor, _proto
from test_gpu_worldpregen import CASES, POSE, _all_same, _frames_and_queries, _replay, _world, host_cells, occupied
from yetanotherconsolegameengine_amd import abi, world_file as wf
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

pytestmark = pytest.mark.gpu

I32P = C.POINTER(C.c_int32)
FORMS = ("fields", "cells")
NO_STORE = "no world store loaded"


def _with_env(env, make):
    """a renderer made with these knobs set (they are read when the context is made)"""
    before = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return make()
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _generate(r, name, form):
    S, cy, cx, cz, seed, ox, oz = CASES[name]
    return r.GenerateWorldStore(_world(name), cx, cz, origin=(ox, oz), form=form)


def _store_proto(name, pairs=ALL_PAIRS, default_material=-1):
    """proto.min_corner is WorldMin: the window's middle over the world's origin, as test_gpu_worldpregen places it"""
    proto, keep = _proto(pairs, default_material)
    w = _world(name)
    proto.min_corner = abi.Vec3(w.world_min.x, w.world_min.y, w.world_min.z)
    return proto, keep


def _chunk(cells, S, key):
    return np.ascontiguousarray(cells[key[0] * S:(key[0] + 1) * S, key[1] * S:(key[1] + 1) * S, key[2] * S:(key[2] + 1) * S])


def _mixed_keys(lib, name, seed=5):
    """all chunks in a drawn order, then a key outside the world, a negative key, an all-Air chunk and an occupied chunk named again"""
    S, cy, cx, cz = CASES[name][:4]
    occ = occupied(host_cells(lib, name), S)
    keys = [(x, y, z) for x in range(cx) for y in range(cy) for z in range(cz)]
    order = np.random.default_rng(seed).permutation(len(keys))
    keys = [keys[i] for i in order]
    air, solid = next(k for k in keys if not occ[k]), next(k for k in keys if occ[k])
    return keys + [(cx, 0, 0), (0, -1, 0), air, solid], len(order)


def _grids_same(A, ia, B, ib, S, keys, label):
    for k, a, b in zip(keys, ia, ib):
        assert (a >= 0) == (b >= 0), (label, k)
        if a < 0:
            continue
        (ra, ma), (rb, mb) = A.read_grid(a, (S, S, S)), B.read_grid(b, (S, S, S))
        assert ra.tobytes() == rb.tobytes() and ma.tobytes() == mb.tobytes(), (label, k)


def _resident(idx):
    return [i for i in idx if i >= 0]


# ---------------------------------------------------------------- 1. store contents
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(CASES))
def test_store_contents(product_lib, name, form):
    S, cy, cx, cz, seed, ox, oz = CASES[name]
    host = host_cells(product_lib, name)
    r = RaytraceRenderer(None, 32, 16)
    assert _generate(r, name, form) == host.shape[:3]
    dims, got_S, occ = r.WorldInfo()
    want = occupied(host, S)
    assert dims == host.shape[:3] and got_S == S and occ.shape == (cx, cy, cz)
    assert occ.astype(bool).tobytes() == want.tobytes() and not want.all()          # every window has a chunk of nothing but Air
    keys = [(x, y, z) for x in range(cx) for y in range(cy) for z in range(cz)]
    if name == "forest4":          # 8 192 chunks: all chunks of two chunk columns - one with an all-Air chunk under an occupied one - and 200 drawn
        gaps = ~want & np.maximum.accumulate(want[:, ::-1], axis=1)[:, ::-1]
        gx, _, gz = (int(v) for v in np.argwhere(gaps)[0])
        drawn = np.random.default_rng(17).choice(len(keys), 200, replace=False)
        keys = [(gx, y, gz) for y in range(cy)] + [(cx - 1, y, 0) for y in range(cy)] + [keys[i] for i in drawn]
    for key in keys:
        got = r.world_store_chunk(*key)
        assert got.shape == (S, S, S, 2) and got.tobytes() == _chunk(host, S, key).tobytes(), (name, form, key)
    gs = r.world_store_generate_stats()
    assert gs["form"] == abi.WORLD_STORE_FORMS[form] and gs["on_host"] == 0
    assert gs["any_leaves_passes"] >= (2 if name == "fallback" else 1)          # "fallback" holds a tree with anyLeaves == false: its flag flips in pass 1
    assert gs["plane_slabs"] == (1 if form == "cells" else 0)
    r.close()


# ---------------------------------------------------------------- 2. read
def _made(kind, lib, name, env=None):
    S = CASES[name][0]
    r = _with_env(env or {}, lambda: RaytraceRenderer(None, 32, 16))
    if kind == "loaded":
        r.LoadWorld(host_cells(lib, name), S)
    else:
        _generate(r, name, kind)
    return r


@pytest.mark.parametrize("memory", ["ordinary", "page_locked"])
@pytest.mark.parametrize("kind", ["fields", "cells", "loaded"])
@pytest.mark.parametrize("name", ["forest", "shore"])          # nx = 64 and 36: neither a multiple of 5
def test_read_gives_the_host_cells(product_lib, name, kind, memory):
    host = host_cells(product_lib, name)
    nx, ny, nz = host.shape[:3]
    assert nx % 5 != 0
    r = _made(kind, product_lib, name)

    def read(x0, planes):
        if memory == "ordinary":
            return r.ReadWorldCells(x0, planes)
        buf, owner = r._page_locked_zeros(((nx - x0) if planes is None else planes, ny, nz, 2), np.int32)
        buf[...] = -9
        return r.ReadWorldCells(x0, planes, out=buf).copy()

    whole = read(0, None)
    assert whole.shape == host.shape and whole.tobytes() == host.tobytes(), int((whole != host).sum())
    for x in range(nx):
        assert read(x, 1).tobytes() == host[x:x + 1].tobytes(), (kind, x)
    for x0 in range(0, nx, 5):
        px = min(5, nx - x0)
        assert read(x0, px).tobytes() == host[x0:x0 + px].tobytes(), (kind, x0)
    r.close()


@pytest.mark.parametrize("kind", ["fields", "cells"])
def test_slabs_of_seven_planes_give_the_same_store_and_the_same_read(product_lib, kind):
    """YCGE_WORLD_STORE_SLAB_BYTES at seven x-planes (and a few bytes: whole planes only): the CELLS form writes the store in ten slabs,
    the last of one plane, and a read of a fields store makes its planes in as many device slabs."""
    name = "forest"
    host = host_cells(product_lib, name)
    nx, ny, nz = host.shape[:3]
    r = _made(kind, product_lib, name, {"YCGE_WORLD_STORE_SLAB_BYTES": 7 * ny * nz * 8 + 5})
    assert r.world_store_generate_stats()["plane_slabs"] == (-(-nx // 7) if kind == "cells" else 0)
    assert r.WorldInfo()[2].astype(bool).tobytes() == occupied(host, CASES[name][0]).tobytes()
    assert r.ReadWorldCells().tobytes() == host.tobytes()
    assert r.ReadWorldCells(3, 20).tobytes() == host[3:23].tobytes()
    r.close()


@pytest.mark.parametrize("kind", ["fields", "cells", "loaded"])
def test_save_resident_writes_the_file_write_vg01_writes(product_lib, tmp_path, kind):
    name = "forest"
    S = CASES[name][0]
    host = host_cells(product_lib, name)
    r = _made(kind, product_lib, name)
    assert wf.save_resident(r, tmp_path / "got.vg", slab_planes=3) == host.shape[:3]          # 64 = 21 x 3 + 1
    wf.write_vg01(tmp_path / "want.vg", host)
    assert (tmp_path / "got.vg").read_bytes() == (tmp_path / "want.vg").read_bytes()
    occ = r.WorldInfo()[2]
    assert r.LoadWorld(tmp_path / "got.vg", S) == host.shape[:3]
    assert r.WorldInfo()[2].tobytes() == occ.tobytes() == occupied(host, S).astype(np.uint8).tobytes()
    r.close()


# ---------------------------------------------------------------- 3. attach
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("in_flight", [0, 2])
@pytest.mark.parametrize("name", ["forest", "fallback"])
def test_attach_equals_an_attach_from_a_store_loaded_with_the_host_cells(product_lib, name, in_flight, form):
    S = CASES[name][0]
    host = host_cells(product_lib, name)
    keys, n_all = _mixed_keys(product_lib, name)
    proto, keep = _store_proto(name)
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    _generate(A, name, form)
    B.LoadWorld(host, S)
    for r in (A, B):
        r.SetCamera(*POSE)
        for _ in range(in_flight):
            r.RenderAsync()
    ia, ib = A.AttachWorldChunks(keys, proto), B.AttachWorldChunks(keys, proto)
    occ = occupied(host, S)
    assert ia == ib
    assert [i >= 0 for i in ia[:n_all]] == [bool(occ[k]) for k in keys[:n_all]]
    assert ia[n_all:n_all + 3] == [-1, -1, -1] and ia[n_all + 3] >= 0 and ia[n_all + 3] not in ia[:n_all]          # outside, negative, all Air; named again: a grid of its own
    n = int(occ.sum()) + 1
    assert sorted(_resident(ia)) == list(range(n))
    sa = A.world_store_stats()
    assert sa["device_chunks"] == n and sa["host_chunks"] == 0
    _grids_same(A, ia, B, ib, S, keys, (name, form))
    fa, fb = _frames_and_queries(A, _resident(ia)), _frames_and_queries(B, _resident(ib))
    _all_same(fa, fb, "generated store against loaded store")
    assert (np.asarray(fa[2][1])[:, 0] >= 0).any() and np.asarray(fa[2][2]).any()          # (the downward rays do meet the chunks)
    A.close(); B.close()


# ---------------------------------------------------------------- 4. sub-batches
def test_sub_batches_of_one_chunk_give_the_same_grids(product_lib):
    """YCGE_ENC_GROUP_BYTES below two chunks' raw cells: every fill launch holds ONE chunk, so a canopy that crosses a chunk border is made in
    another sub-batch than its root."""
    name = "forest"
    S = CASES[name][0]
    host = host_cells(product_lib, name)
    keys, n_all = _mixed_keys(product_lib, name)
    proto, keep = _store_proto(name)
    A = _with_env({"YCGE_ENC_GROUP_BYTES": S * S * S * 8 + 1000}, lambda: RaytraceRenderer(_anchor(), 32, 16))
    B = RaytraceRenderer(_anchor(), 32, 16)
    _generate(A, name, "fields")
    B.LoadWorld(host, S)
    ia, ib = A.AttachWorldChunks(keys, proto), B.AttachWorldChunks(keys, proto)
    assert ia == ib
    _grids_same(A, ia, B, ib, S, keys, "sub-batches")
    A.close(); B.close()


# ---------------------------------------------------------------- 5. streaming
def test_streaming_ticks_equal_those_of_a_loaded_store(product_lib):
    name = "forest"
    S, cy, cx, cz = CASES[name][:4]
    host = host_cells(product_lib, name)
    proto, keep = _store_proto(name)
    A = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    _generate(A, name, "fields")
    B.LoadWorld(host, S)
    wmin = (proto.min_corner.x, proto.min_corner.y, proto.min_corner.z)
    centres = [(-30.5, 60.0, -30.5), (-14.5, 60.0, -30.5), (-14.5, 60.0, -14.5), (1.5, 60.0, -14.5), (1.5, 60.0, 1.5), (17.5, 60.0, 17.5)]
    columns = [wf.center_column(c, wmin, (1, 1, 1), S) for c in centres]
    assert len({c[0] for c in columns}) >= 3 and len({c[1] for c in columns}) >= 3          # the walk crosses chunk borders in x and in z
    la, lb = {}, {}
    for step, centre in enumerate(centres):
        ta = wf.stream_resident(A, proto, centre, S, 1, cy, la)
        tb = wf.stream_resident(B, proto, centre, S, 1, cy, lb)
        assert ta == tb and la == lb, step
        assert step == 0 or (ta[0] and ta[1])          # every later tick attaches and drops chunks
        _grids_same(A, [la[k] for k in ta[0]], B, [lb[k] for k in tb[0]], S, ta[0], f"streaming step {step}")
        for k in ta[0]:          # ... and both hold the host generator's cells, through the lookup of test_gpu_worldgen._proto
            if la[k] >= 0:
                part = _chunk(host, S, k)
                want = np.where(part[..., 0] > 0, (part[..., 0] * 3 + part[..., 1]) % 27, -1)
                assert (A.read_grid(la[k], (S, S, S))[1] == want).all() and (B.read_grid(lb[k], (S, S, S))[1] == want).all(), (step, k)
        fa, fb = _frames_and_queries(A, _resident(la.values())), _frames_and_queries(B, _resident(lb.values()))
        _all_same(fa, fb, f"streaming step {step}")
        A.DetachGrids(ta[2]); B.DetachGrids(tb[2])
    assert A.world_store_stats()["device_chunks"] == B.world_store_stats()["device_chunks"] > 0
    A.close(); B.close()


# ---------------------------------------------------------------- 6. replace and release
def _info_and_chunks(r, keys):
    dims, S, occ = r.WorldInfo()
    return dims, S, occ.tobytes(), [r.world_store_chunk(*k).tobytes() for k in keys]


def test_replace_and_release(product_lib):
    L = product_lib
    n1, n2 = "small", "shore"
    S1, S2 = CASES[n1][0], CASES[n2][0]
    h1, h2 = host_cells(L, n1), host_cells(L, n2)
    proto, keep = _store_proto(n1)
    some = [(0, 0, 0), (2, 3, 1), (4, 5, 3)]
    r = RaytraceRenderer(_anchor(), 96, 27, 60.0)
    # a generate replaces a loaded store
    r.LoadWorld(h2, S2)
    _generate(r, n1, "fields")
    info = _info_and_chunks(r, some)
    assert info[:3] == (h1.shape[:3], S1, occupied(h1, S1).astype(np.uint8).tobytes()) and info[3] == [_chunk(h1, S1, k).tobytes() for k in some]
    keys = [(x, y, z) for x in range(CASES[n1][2]) for y in range(CASES[n1][1]) for z in range(CASES[n1][3])]
    idx = _resident(r.AttachWorldChunks(keys, proto))
    first = _replay(r, idx)
    # a refused generate leaves the old store as it was, byte for byte
    S, cy, cx, cz, seed, ox, oz = CASES[n1]
    w = _world(n1)
    lim = 1 << 24
    for a, b, x, z, form in ((0, cz, ox, oz, 0), (cx, cz, lim, oz, 0), (cx, cz, ox, -lim - 1, 1), (cx, cz, ox, oz, 2)):
        assert L.ycge_world_store_generate(r.ctx, C.byref(w), a, b, x, z, form) == abi.YCGE_ERR_INVALID_ARG, (a, b, x, z, form)
        assert L.ycge_last_error(r.ctx).startswith(b"ycge_world_store_generate")
    assert _info_and_chunks(r, some) == info
    # a load replaces a generated store, a generate of the other form replaces that
    r.LoadWorld(h2, S2)
    assert r.WorldInfo()[0] == h2.shape[:3] and r.world_store_chunk(1, 2, 1).tobytes() == _chunk(h2, S2, (1, 2, 1)).tobytes()
    _generate(r, n1, "cells")
    assert _info_and_chunks(r, some) == info
    _all_same(first, _replay(r, idx), "after the store was replaced three times")
    r._check(L.ycge_scene_upload(r.ctx, r.flat.byref()))          # the store is not scene state
    assert r.WorldInfo()[0] == h1.shape[:3]
    idx = _resident(r.AttachWorldChunks(keys, proto))
    first = _replay(r, idx)
    # release: an attach and a read are refused as they are with no store; the grids stay
    _generate(r, n1, "fields")
    r.ReleaseWorld()
    assert r.world_store_stats()["store_bytes"] == 0
    out = np.full(len(keys), -7, np.int32)
    karr = np.ascontiguousarray(np.asarray(keys, np.int32))
    assert L.ycge_scene_attach_world_chunks(r.ctx, karr.ctypes.data_as(I32P), len(keys), C.byref(proto), out.ctypes.data_as(I32P)) == abi.YCGE_ERR_INVALID_ARG
    assert NO_STORE.encode() in L.ycge_last_error(r.ctx) and (out == -7).all()
    plane = np.full((1,) + h1.shape[1:], -9, np.int32)
    assert L.ycge_world_store_read(r.ctx, 0, 1, plane.ctypes.data) == abi.YCGE_ERR_INVALID_ARG
    assert NO_STORE.encode() in L.ycge_last_error(r.ctx) and (plane == -9).all()
    _all_same(first, _replay(r, idx), "after the store was released")
    r.close()


# ---------------------------------------------------------------- 7. refusals
def test_refusals_write_nothing(product_lib):
    L = product_lib
    name = "small"
    S, cy, cx, cz, seed, ox, oz = CASES[name]
    w = _world(name)
    host = host_cells(L, name)
    nx, ny, nz = host.shape[:3]
    r = RaytraceRenderer(_anchor(), 160, 90, devices=[0, 0])
    gen = lambda ctx, world, a, b, x, z, form: L.ycge_world_store_generate(ctx, C.byref(world) if world is not None else None, a, b, x, z, form)
    # with no store: every refusal of generate leaves none
    lim = 1 << 24
    bad_world = abi.World(3, cy, seed, w.world_min, w.voxel_size)
    huge = abi.World(64, 16, 0, w.world_min, w.voxel_size)
    cases = [(bad_world, cx, cz, ox, oz, 0), (None, cx, cz, ox, oz, 0), (w, 0, cz, ox, oz, 0), (w, cx, 0, ox, oz, 0), (w, -1, cz, ox, oz, 1), (w, cx, cz, lim, oz, 0),
             (w, cx, cz, ox, -lim - 1, 1), (w, cx, cz, -lim - 1, oz, 0), (huge, 16, 16, 0, 0, 0), (w, cx, cz, ox, oz, -1), (w, cx, cz, ox, oz, 2)]
    for case in cases:
        assert gen(r.ctx, *case) == abi.YCGE_ERR_INVALID_ARG, case[1:]
        assert L.ycge_last_error(r.ctx).startswith(b"ycge_world_store_generate: ")
        assert L.ycge_world_store_info(r.ctx, None, None, None, 0) == abi.YCGE_ERR_INVALID_ARG and NO_STORE.encode() in L.ycge_last_error(r.ctx)
    peer = C.c_void_p(L.ycge_debug_peer_context(r.ctx, 0))
    assert peer.value
    assert gen(peer, w, cx, cz, ox, oz, 0) == abi.YCGE_ERR_INVALID_ARG and b"driven by their root" in L.ycge_last_error(peer)
    assert gen(None, w, cx, cz, ox, oz, 0) == abi.YCGE_ERR_INVALID_ARG
    buf = np.full((nx + 1, ny, nz, 2), -9, np.int32)
    assert L.ycge_world_store_read(r.ctx, 0, 1, buf.ctypes.data) == abi.YCGE_ERR_INVALID_ARG and NO_STORE.encode() in L.ycge_last_error(r.ctx)
    # with a store of each kind: the refusals of read, and of generate again
    for kind in ("fields", "cells", "loaded"):
        if kind == "loaded":
            r.LoadWorld(host, S)
        else:
            _generate(r, name, kind)
        info = _info_and_chunks(r, [(1, 2, 3)])
        for x0, planes in ((-1, 1), (0, 0), (0, -3), (nx, 1), (nx - 1, 2), (0, nx + 1), (2 ** 31 - 1, 2), (1, 2 ** 31 - 1)):
            assert L.ycge_world_store_read(r.ctx, x0, planes, buf.ctypes.data) == abi.YCGE_ERR_INVALID_ARG, (kind, x0, planes)
            assert L.ycge_last_error(r.ctx).startswith(b"ycge_world_store_read: ")
        assert L.ycge_world_store_read(r.ctx, 0, 1, None) == abi.YCGE_ERR_INVALID_ARG
        assert L.ycge_world_store_read(peer, 0, 1, buf.ctypes.data) == abi.YCGE_ERR_INVALID_ARG and b"driven by their root" in L.ycge_last_error(peer)
        assert L.ycge_world_store_read(None, 0, 1, buf.ctypes.data) == abi.YCGE_ERR_INVALID_ARG
        for case in cases:
            assert gen(r.ctx, *case) == abi.YCGE_ERR_INVALID_ARG
        assert gen(peer, w, cx, cz, ox, oz, 1) == abi.YCGE_ERR_INVALID_ARG
        assert (buf == -9).all() and _info_and_chunks(r, [(1, 2, 3)]) == info, kind
        assert r.ReadWorldCells(nx - 1, 1).tobytes() == host[nx - 1:].tobytes()          # the last plane is there to be read
    r.close()


# ---------------------------------------------------------------- 8. knobs
@pytest.mark.parametrize("knob", ["YCGE_WORLDGEN_HOST", "YCGE_WORLD_STORE_HOST", "large_lookup"])
def test_the_knobs_give_the_same_indices_grids_and_frames(product_lib, knob):
    name = "fallback"
    S = CASES[name][0]
    host = host_cells(product_lib, name)
    keys, n_all = _mixed_keys(product_lib, name)
    pairs = ALL_PAIRS + ([(100 + i, 0) for i in range(280)] if knob == "large_lookup" else [])
    proto, keep = _store_proto(name, pairs)
    K = _with_env({knob: 1} if knob != "large_lookup" else {}, lambda: RaytraceRenderer(_anchor(), 96, 27, 60.0))
    B = RaytraceRenderer(_anchor(), 96, 27, 60.0)          # the yardstick: a store loaded with the host cells
    _generate(K, name, "fields")
    B.LoadWorld(host, S)
    assert K.WorldInfo()[2].tobytes() == B.WorldInfo()[2].tobytes()
    assert K.ReadWorldCells().tobytes() == host.tobytes()
    ik, ib = K.AttachWorldChunks(keys, proto), B.AttachWorldChunks(keys, proto)
    assert ik == ib
    n = len(_resident(ik))
    gs, ws, pool = K.world_store_generate_stats(), K.world_store_stats(), K.grid_pool_stats()
    if knob == "YCGE_WORLDGEN_HOST":          # the host generator's cells in the ordinary device store: sliced by k_ws_slice
        assert gs["on_host"] == 1 and gs["host_generator_us"] > 0 and (ws["device_chunks"], ws["host_chunks"]) == (n, 0) and ws["store_bytes"] == host.nbytes
    elif knob == "YCGE_WORLD_STORE_HOST":     # ... in a host copy: sliced by the host loop
        assert gs["on_host"] == 1 and (ws["device_chunks"], ws["host_chunks"]) == (0, n) and ws["store_bytes"] == host.nbytes
    else:                                     # a fields store whose chunks the host encoder takes: each filled into a buffer of its own and copied out
        assert gs["on_host"] == 0 and (ws["device_chunks"], ws["host_chunks"]) == (0, n) and (pool["host_encodes"], pool["device_encodes"]) == (n, 0)
    _grids_same(K, ik, B, ib, S, keys, knob)
    _all_same(_frames_and_queries(K, _resident(ik)), _frames_and_queries(B, _resident(ib)), knob)
    K.close(); B.close()


# ---------------------------------------------------------------- 9. two devices
@pytest.mark.parametrize("form", FORMS)
def test_two_devices_give_the_indices_and_frames_of_one(product_lib, form):
    """A context that drives two devices (both own tiles at 160 x 90) on the window whose anyLeaves passes number two at least: the peer
    repeats the root's passes without reading anything back, and fills its own chunks from its own fields."""
    name = "fallback"
    keys, n_all = _mixed_keys(product_lib, name)
    proto, keep = _store_proto(name)

    def run(devices):
        r = RaytraceRenderer(_anchor(), 160, 90, devices=devices)
        _generate(r, name, form)
        assert r.world_store_generate_stats()["any_leaves_passes"] >= 2
        idx = r.AttachWorldChunks(keys, proto)
        out = _frames_and_queries(r, _resident(idx))[:2]
        r.close()
        return idx, out

    (i1, one), (i2, two) = run(None), run([0, 0])
    assert i1 == i2
    _all_same(one, two, "two devices against one")


# ---------------------------------------------------------------- 10. footprint
def test_the_fields_store_is_a_fraction_of_the_cells(product_lib):
    """128 cells of 8 bytes a column against tens of bytes of fields a column"""
    name = "forest"
    host = host_cells(product_lib, name)
    nx, ny, nz = host.shape[:3]
    r = RaytraceRenderer(None, 32, 16)
    _generate(r, name, "fields")
    fields = r.world_store_stats()["store_bytes"]
    _generate(r, name, "cells")
    cells = r.world_store_stats()["store_bytes"]
    assert cells == 8 * nx * ny * nz == host.nbytes
    assert 0 < fields < cells // 8, (fields, cells)
    r.close()
