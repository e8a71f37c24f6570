"""-m gpu: voxel edits - ycge_scene_edit_voxels / ycge_world_store_edit (csrc/ycge_grid_edit.*, csrc/ycge_world_store.*).  The reference has no
block editing, so the existing paths define the result: an edited context against a twin that attaches, uploads or loads the cells with
the ops applied by the numpy restatement (tests/voxel_edit_restatement.py).  Every comparison is bit for bit (parity_util.mismatch_count == 0)."""
import ctypes as C
import os

import numpy as np
import pytest

import parity_util as pu
import voxel_edit_restatement as ve
from yetanotherconsolegameengine_amd import abi, scenes, world_file
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import AmbientLight, Material, Scene, Sphere, VolumeGrid, ZERO, flatten, vec3

pytestmark = pytest.mark.gpu

CHUNK, VIEW = 32, 1
WORLD_MIN, VOXEL = (-48.0, 0.0, -48.0), (1.0, 1.0, 1.0)
PATH = [(0.0, 0.0), (10.0, 0.0), (20.0, 3.0), (40.0, 3.0), (40.0, 20.0), (40.0, 40.0), (5.0, 5.0)]          # the first ticks of test_gpu_grid_stream's walk
FRAME_BUFFERS = (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY, abi.BUF_PREV_NORMAL,
                 abi.BUF_PREV_DEPTH, abi.BUF_PREV_SKY, abi.BUF_DENOISED)
DEBUG_BUFFERS = (abi.BUF_RAYS, abi.BUF_PRIM_ID, abi.BUF_SUB_ID, abi.BUF_HIT_T, abi.BUF_RNG_STATE)
COUNTERS = ("n_rays", "n_box", "n_tri", "n_prim", "n_vox", "n_rays_dark")


def _same(a, b, label):
    assert a.shape == b.shape, label
    n = pu.mismatch_count(a, b)
    assert n == 0, f"{label}: {n} elements differ"


def _same_buffers(g, t, buffers, label):
    for which in buffers:
        _same(g.read(which), t.read(which), f"{label}: buffer {which}")


def _record_fields(rec):
    """the GGrid record with cell_offset (word 12) and lut_offset (word 16) blanked"""
    w = rec.view(np.uint32).copy()
    w[12] = 0; w[16] = 0
    return w


def _with_env(env, make):
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


_ANCHOR = {}


def _anchor():
    """a scene of N_MATERIALS small spheres: every material of the restatement's palette is a material of the upload, material k at index k"""
    if not _ANCHOR:
        rng = np.random.default_rng(4)
        s = Scene()
        s.Ambient = AmbientLight(vec3(1, 1, 1), 0.3)
        for k in range(ve.N_MATERIALS):
            s.Add(Sphere(vec3(-3.0 + 0.5 * k, 0.5, -6.0), 0.2, Material(vec3(*rng.uniform(0.1, 0.9, 3)), 0.1, 0.0, ZERO)))
        fa = flatten(s)
        mats = [o.Mat for o in s.Objects]
        assert [fa._mat_index[id(m)] for m in mats] == list(range(ve.N_MATERIALS))
        _ANCHOR["scene"], _ANCHOR["flat"] = s, fa
    return _ANCHOR["flat"]


def _record(cells, corner, voxel, keep, n_lookup=None, default=ve.DEFAULT_MATERIAL, pairs=ve.PALETTE):
    """a ycge_grid over `cells` with the restatement's lookup table (padded with unused entries to n_lookup) and default material"""
    cells = np.ascontiguousarray(cells, np.int32)
    n = max(len(pairs), n_lookup or 0)
    lut = (abi.VoxelLookup * max(1, n))()
    for i in range(n):
        lut[i].mat_id, lut[i].meta_id, lut[i].material = (*pairs[i], i % ve.N_MATERIALS) if i < len(pairs) else (100000 + i, 0, i % ve.N_MATERIALS)
    keep += [cells, lut]
    g = abi.Grid()
    g.nx, g.ny, g.nz = cells.shape[:3]
    g.min_corner, g.voxel_size = abi.Vec3(*corner), abi.Vec3(*voxel)
    g.cells, g.lookup, g.n_lookup = cells.ctypes.data_as(C.POINTER(C.c_int32)), C.cast(lut, C.POINTER(abi.VoxelLookup)), n
    g.default_material, g.wireframe, g.wire_width_fraction, g.wire_max_distance = default, 1, 0.06, 16.0
    return g


def _attach(r, rec):
    out = (C.c_int32 * 1)(-7)
    r._check(r.L.ycge_scene_attach_grids(r.ctx, (abi.Grid * 1)(rec), 1, out))
    return int(out[0])


def _holder(form, cells, corner, voxel, keep, **kw):
    """a renderer that holds the grid at index 0: attached (the device encoded it), inside an upload, or attached with a lookup table above 254 entries (host-encoded both)"""
    fa = _anchor()
    if form == "uploaded":
        sc = abi.Scene()
        C.memmove(C.byref(sc), C.byref(fa.struct), C.sizeof(sc))
        arr = (abi.Grid * 1)(_record(cells, corner, voxel, keep))
        keep.append(arr)
        sc.grids, sc.n_grids = C.cast(arr, C.POINTER(abi.Grid)), 1
        r = RaytraceRenderer(None, 32, 16, **kw)
        r._check(r.L.ycge_scene_upload(r.ctx, C.byref(sc)))
        return r
    r = RaytraceRenderer(fa, 32, 16, **kw)
    assert _attach(r, _record(cells, corner, voxel, keep, n_lookup=300 if form == "large lookup" else None)) == 0
    st = r.grid_pool_stats()
    assert (st["device_encodes"], st["host_encodes"]) == ((1, 0) if form == "attached" else (0, 1)), (form, st)
    return r


# ------------------------------------------------------------------------------------------------ 1. encoder equality
def _edit_against_attach(labels, forms, **kw):
    grids = ve.drawn_grids()
    twin = RaytraceRenderer(_anchor(), 32, 16)
    for label in labels:
        cells, corner, voxel = grids[label]
        calls = ve.drawn_calls(label, cells)
        for form in forms:
            keep = []
            r = _holder(form, cells, corner, voxel, keep, **kw)
            now = cells
            for k, ops in enumerate(calls):
                info = r.EditVoxels(ops)
                after = ve.apply_ops(now, ops)
                where = f"{label}, {form}, call {k}"
                want = ve.expected_info(now, after, host_encoded=form != "attached")
                assert (info["cells_changed"], info["bricks_written"], info["records_changed"], info["objects_installed"]) == want + (0,), (where, info, want)
                ti = _attach(twin, _record(after, corner, voxel, keep))
                (ra, ma), (rb, mb) = r.read_grid(0, cells.shape[:3]), twin.read_grid(ti, cells.shape[:3])
                twin._check(twin.L.ycge_scene_detach_grids(twin.ctx, (C.c_int32 * 1)(ti), 1))
                _same(ma, mb, f"{where}: per-voxel materials")
                _same(ma, ve.materials_of(after), f"{where}: materials of the restatement")
                _same(_record_fields(ra), _record_fields(rb), f"{where}: record")
                now = after
            r.close()
    twin.close()


@pytest.mark.parametrize("form", ["attached", "uploaded", "large lookup"])
def test_edited_grids_equal_an_attach_of_the_edited_cells(product_lib, form):
    _edit_against_attach(list(ve.drawn_grids()), [form])


# ------------------------------------------------------------------------------------------------ 2. frames
def _world_scene(t01=0.5):
    world = scenes.make_voxel_world(96, 128, 96)
    s = Scene()
    s.IsVolumeScene = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.0)
    lights, top, bottom = scenes.sun_moon_lights(t01)
    s.Lights.extend(lights)
    s.BackgroundTop, s.BackgroundBottom = top, bottom
    return s, world


def _tick(scene, world, loaded, cache, x, z):
    return world_file.stream_view(scene, world, (x, 70.0, z), WORLD_MIN, VOXEL, CHUNK, VIEW, scenes.VoxelMaterialLookup, loaded, cache=cache)


def _pose(x, z):
    return dict(pos=(float(x), 70.0, float(z)), yaw=0.4, pitch=-0.45, fov=60.0)


def _edit_world(g, chunks, held, ops):
    """World-cell ops applied to the Python VolumeGrids of `chunks` (key -> VolumeGrid: what the twin uploads) and, as chunk-local boxes, to
    their resident grids.  Returns (EditVoxels' info, whether the restatement says a held grid's box or mask changed)."""
    local = world_file.clip_ops_to_chunks(ops, list(chunks), CHUNK)
    rows, reinstall = [], False
    for key, boxes in local.items():
        vg = chunks[key]
        mine = [[g.flat._grid_index[id(vg)], *b] for b in boxes]
        after = ve.apply_ops(vg.Cells, mine)
        reinstall |= key in held and ve.record_changed(vg.Cells, after)
        vg.Cells = after
        rows += mine
    assert rows
    return g.EditVoxels(rows), reinstall


def _highest_column(world, columns):
    """(x, top y + 1, z) of the highest column of the first chunk column (cx, cz) of `columns` whose highest chunk has room above every column:
    a pillar on it raises that chunk's solid box"""
    for cx, cz in columns:
        part = world[32 * cx:32 * cx + 32, :, 32 * cz:32 * cz + 32, 0] > 0
        tops = part.shape[1] - np.argmax(part[:, ::-1, :], axis=1)          # per column: its highest solid cell + 1
        h = int(tops.max())
        if h % 32 >= 2:
            x, z = np.argwhere(tops == h)[0]
            return 32 * cx + int(x), h, 32 * cz + int(z)
    raise AssertionError("no such column")


def _down_rays(cols):
    org = np.array([[WORLD_MIN[0] + x + 0.5 + dx, 127.5, WORLD_MIN[2] + z + 0.5 + dz] for x, z in cols for dx, dz in ((0, 0), (0.3, -0.2), (-1.2, 0.4))], np.float32)
    d = np.tile(np.array([[0.01, -1.0, 0.02]], np.float32), (len(org), 1))
    return org, d


@pytest.mark.parametrize("counting", [True, False], ids=["counting", "timed"])
def test_edits_between_ticks_equal_the_uploading_twin(product_lib, counting):
    scene, world = _world_scene()
    loaded, cache = {}, {}
    _tick(scene, world, loaded, cache, *PATH[0])
    first = list(scene.Objects)          # the upload holds half of the first view (host-encoded slots), the walk attaches the rest (device-encoded)
    scene.Objects[:] = first[:len(first) // 2]
    for k in [k for k, v in loaded.items() if not any(v is o for o in scene.Objects)]:
        del loaded[k]
    kw = dict(capture_debug=counting, count_work=counting)
    g = RaytraceRenderer(flatten(scene), 96, 54, 60.0, 1, **kw)
    t = RaytraceRenderer(flatten(scene), 96, 54, 60.0, 1, **kw)
    px, ph, pz = _highest_column(world, [(1, 1), (2, 1), (1, 0), (2, 0), (1, 2), (2, 2)])          # (columns that stay in view over ticks 2 and 3)
    qh = int(np.flatnonzero(world[61, :, 61, 0] > 0).max()) + 1
    pillar_pair = tuple(int(v) for v in world[px, ph - 1, pz])
    top = 32 * (ph // 32 + 1) - 1
    plan = {                                                                    # tick -> world-cell ops
        1: [ve.op((50, 40, 50), (51, 120, 51), (0, 0)), ve.op((44, 70, 44), (44, 70, 44), (-2, 3))],      # a dug shaft through three chunks of the centre column
        2: [ve.op((px, ph, pz), (px, top, pz), pillar_pair)],                   # a pillar up to its chunk's top: the box rises
        3: [ve.op((px, ph, pz), (px, top, pz), (0, 0))],                        # ... and goes again: it shrinks
        5: [ve.op((5, 50, 5), (9, 127, 9), (0, 0))],                            # a shaft in a corner column that has left the view: cached, unreferenced
        6: [ve.op((60, qh - 2, 60), (61, qh - 1, 61), (0, 0)), ve.op((61, qh - 1, 61), (61, qh - 1, 61), tuple(int(v) for v in world[61, qh - 1, 61]))],          # the later op wins
    }
    installs = []
    for tick, (x, z) in enumerate(PATH):
        _tick(scene, world, loaded, cache, x, z)
        g.StreamObjects(scene, keep_cached=True)
        if tick in plan:
            chunks = {**cache, **loaded}
            if tick == 5:
                assert (0, 1, 0) in cache and (0, 1, 0) not in loaded
            info, reinstall = _edit_world(g, chunks, loaded, plan[tick])
            assert info["objects_installed"] == int(reinstall), (tick, info, reinstall)
            assert info["cells_changed"] > 0, (tick, info)
            installs.append(info["objects_installed"])
        t.UploadScene(flatten(scene))
        p = _pose(x, z)
        for r in (g, t):
            r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        for f in range(2):
            label = f"tick {tick} frame {f}"
            _same(g.TryFlipAndBlit(want_sdr=True), t.TryFlipAndBlit(want_sdr=True), f"{label}: SDR frame")
            _same_buffers(g, t, FRAME_BUFFERS + (DEBUG_BUFFERS if counting else ()), label)
            if counting:
                for k in COUNTERS:
                    assert getattr(g.stats, k) == getattr(t.stats, k), (label, k)
            else:
                assert g.timed_steps() == t.timed_steps(), label
        org, d = _down_rays([(50, 50), (px, pz), (5, 5), (61, 61), (44, 44)])
        (hg, ig), (ht, it) = g.Hit(org, d), t.Hit(org, d)
        _same(ig, it, f"tick {tick}: ids of rays through the edited cells"); _same(hg, ht, f"tick {tick}: their hits")
        _same(g.Occluded(org, d), t.Occluded(org, d), f"tick {tick}: occlusion")
    assert installs[1] == 1 and installs[2] == 1 and 0 in installs, installs          # the pillar changes its chunk's box both ways; some edit changes no record of a held grid
    g.close(); t.close()


# ------------------------------------------------------------------------------------------------ 3. frames in flight
def test_an_edit_between_frames_in_flight(product_lib):
    watch = (abi.BUF_CURRENT_HDR, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY)

    def run(in_flight):
        scene, world = _world_scene()
        loaded = {}
        _tick(scene, world, loaded, None, *PATH[0])
        r = RaytraceRenderer(flatten(scene), 160, 90, 60.0, 1)
        p = _pose(20.0, 3.0)
        r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        out = []
        for step in range(4):
            if step == 2:
                info, _ = _edit_world(r, loaded, loaded, [ve.op((60, 30, 40), (75, 127, 60), (0, 0))])
                assert info["cells_changed"] > 1000
            if in_flight:
                r.RenderAsync()
                if step in (1, 3):
                    r.Wait()
            else:
                r.TryFlipAndBlit()
            if step in (1, 3):
                out.append([r.read(b) for b in watch])
        r.close()
        return out

    want, got = run(False), run(True)
    for i, (a, b) in enumerate(zip(want, got)):
        for wch, x, y in zip(watch, a, b):
            _same(x, y, f"frames {2 * i}..{2 * i + 1}, buffer {wch}")


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_change_nothing(product_lib):
    L = abi.load_library()
    rng = np.random.default_rng(8)
    cells = np.zeros((13, 9, 21, 2), np.int32)
    cells[..., 0] = rng.integers(0, 4, cells.shape[:3]); cells[..., 1] = 0
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.4)
    for m in [o.Mat for o in (_anchor() and _ANCHOR["scene"]).Objects]:
        s.Add(Sphere(vec3(0, -50, 0), 0.1, m))
    s.Add(VolumeGrid(cells, vec3(-3.0, -1.0, -12.0), vec3(0.5, 0.5, 0.5), lambda a, b: s.Objects[(a + b) % 4].Mat))
    flat = flatten(s)
    g, twin = RaytraceRenderer(flat, 64, 36, 60.0, 1), RaytraceRenderer(flat, 64, 36, 60.0, 1)
    keep = []
    many = np.ones((16, 16, 1, 2), np.int32); many[..., 1] = np.arange(256).reshape(16, 16, 1); many[15, 15, 0] = (0, 0)          # 255 distinct pairs
    shapes = {0: cells.shape[:3]}
    for r in (g, twin):
        i_dev = _attach(r, _record(cells, (0, 0, 0), (1, 1, 1), keep, default=-1))                       # device-encoded, a miss has no material
        i_full = _attach(r, _record(many, (0, 0, 0), (1, 1, 1), keep, n_lookup=300, default=0))          # host-encoded, every code taken
    shapes[i_dev], shapes[i_full] = cells.shape[:3], many.shape[:3]
    assert g.grid_pool_stats()["host_encodes"] == 1

    def ops_of(rows):
        arr = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 9))
        keep.append(arr)
        return arr.ctypes.data

    good = ve.op((0, 0, 0), (1, 1, 1), (1, 0), grid=i_dev)
    info = (C.c_uint32 * 4)(7, 7, 7, 7)

    def refused(ctx, rows, n, status, needle, label):
        before = {i: g.read_grid(i, sh) for i, sh in shapes.items()}
        stats = g.grid_pool_stats()
        rc = L.ycge_scene_edit_voxels(ctx, ops_of(rows) if rows is not None else None, n, info)
        err = L.ycge_last_error(ctx) or b""
        assert rc == status, (label, rc, err)
        assert needle in err, (label, err)
        assert list(info) == [7, 7, 7, 7], label
        assert g.grid_pool_stats() == stats, label
        for i, sh in shapes.items():
            rec, mats = g.read_grid(i, sh)
            _same(rec, before[i][0], f"{label}: record of grid {i}"); _same(mats, before[i][1], f"{label}: materials of grid {i}")
        g.TryFlipAndBlit(); twin.TryFlipAndBlit()
        _same_buffers(g, twin, (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY, abi.BUF_G_DEPTH), label)

    bad = abi.YCGE_ERR_INVALID_ARG
    refused(g.ctx, None, 1, bad, b"bad op array", "NULL ops with n > 0")
    refused(g.ctx, [good], -1, bad, b"bad op array", "n < 0")
    refused(g.ctx, [good], (1 << 20) + 1, bad, b"bad op array", "n > 2^20")
    refused(g.ctx, [good, ve.op((0, 0, 0), (0, 0, 0), (1, 0), grid=40)], 2, bad, b"op 1: grid 40 is not resident", "a grid that is not resident")
    refused(g.ctx, [good, ve.op((0, 3, 0), (0, 2, 0), (1, 0), grid=i_dev)], 2, bad, b"op 1: lo 3 > hi 2 on axis 1", "lo > hi")
    refused(g.ctx, [good, ve.op((0, 0, 0), (0, 0, 21), (1, 0), grid=i_dev)], 2, bad, b"op 1: the box leaves grid", "a box that leaves the grid")
    refused(g.ctx, [good, ve.op((0, 0, -1), (0, 0, 2), (1, 0), grid=0)], 2, bad, b"op 1: the box leaves grid", "a box that begins below 0")
    refused(g.ctx, [good, ve.op((2, 2, 2), (2, 2, 2), (77, 4), grid=i_dev)], 2, bad, b"op 1: no material for (matId 77, metaId 4)", "a solid pair with no material")
    refused(g.ctx, [good, ve.op((2, 2, 2), (2, 2, 2), (77, 4), grid=0)], 2, bad, b"op 1: no material for (matId 77, metaId 4)", "... on a grid of the upload")
    refused(g.ctx, [good, ve.op((0, 0, 0), (0, 0, 0), (1, 999), grid=i_full)], 2, abi.YCGE_ERR_UNSUPPORTED, b"op 1: (matId 1, metaId 999) would be the 256th cell code", "the 256th code")
    assert b"not reclaimed" in L.ycge_last_error(g.ctx)
    # a peer context refuses; a context with no scene has none
    two = RaytraceRenderer(flat, 64, 36, 60.0, 1, devices=[0, 0])
    peer = C.c_void_p(two.L.ycge_debug_peer_context(two.ctx, 0))
    assert peer.value
    before = two.read_grid(0, cells.shape[:3])
    assert L.ycge_scene_edit_voxels(peer, ops_of([ve.op((0, 0, 0), (1, 1, 1), (0, 0))]), 1, info) == bad and b"driven by their root" in L.ycge_last_error(peer)
    assert L.ycge_world_store_edit(peer, ops_of([ve.op((0, 0, 0), (1, 1, 1), (0, 0))]), 1) == bad
    _same(two.read_grid(0, cells.shape[:3])[1], before[1], "a peer's refusal")
    two.close()
    empty = RaytraceRenderer(None, 64, 36, 60.0, 1)
    assert L.ycge_scene_edit_voxels(empty.ctx, ops_of([good]), 1, info) == abi.YCGE_ERR_NO_SCENE
    empty.close()
    assert list(info) == [7, 7, 7, 7]
    # n = 0 is fine, and the good op alone goes through: an existing pair keeps its code on the full grid too
    assert L.ycge_scene_edit_voxels(g.ctx, None, 0, info) == abi.YCGE_OK and list(info) == [0, 0, 0, 0]
    out = g.EditVoxels([good, ve.op((15, 15, 0), (15, 15, 0), (1, 7), grid=i_full)])
    assert out["cells_changed"] >= 1
    assert g.read_grid(i_full, many.shape[:3])[1][15, 15, 0] == 0          # (the pair's code existed: the table lacks it, default_material 0)
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 5. the world store
def _store_proto(keep, world_min=(0.0, 0.0, 0.0)):
    g = _record(np.zeros((1, 1, 1, 2), np.int32), world_min, (1.0, 1.0, 1.0), keep)
    return g


def _stores_agree(a, b, S, label):
    keep = []
    proto = _store_proto(keep)
    (da, sa, oa), (db, sb, ob) = a.WorldInfo(), b.WorldInfo()
    assert (da, sa) == (db, sb), label
    _same(oa, ob, f"{label}: occupancy")
    _same(a.ReadWorldCells(), b.ReadWorldCells(), f"{label}: every plane of the store")
    keys = [(x, y, z) for x in range(oa.shape[0]) for y in range(oa.shape[1]) for z in range(oa.shape[2])]
    ia, ib = a.AttachWorldChunks(keys, proto), b.AttachWorldChunks(keys, proto)
    assert [i >= 0 for i in ia] == [i >= 0 for i in ib] == [bool(oa[k]) for k in keys], label
    for key, i, j in zip(keys, ia, ib):
        if i < 0:
            continue
        shape = tuple(min(S, da[k] - key[k] * S) for k in range(3))
        (ra, ma), (rb, mb) = a.read_grid(i, shape), b.read_grid(j, shape)
        _same(ma, mb, f"{label}: chunk {key}: materials"); _same(_record_fields(ra), _record_fields(rb), f"{label}: chunk {key}: record")
    return oa


def _store_case(form, **kw):
    w, ops, S = ve.store_world(), ve.store_ops(), ve.STORE_CHUNK
    make = lambda: RaytraceRenderer(_anchor(), 32, 16, **kw)
    a = _with_env({"YCGE_WORLD_STORE_HOST": 1}, make) if form == "host" else make()
    b = make()
    if form == "generated":
        world = abi.World(16, 2, 11, abi.Vec3(0, 0, 0), abi.Vec3(1, 1, 1))
        a.GenerateWorldStore(world, 2, 2, form="cells")
        w = a.ReadWorldCells().copy()
        solid = np.argwhere(w[..., 0] != 0)
        assert len(solid) and w.shape[:3] == (32, 32, 32)
        ops = [ve.op((0, 0, 0), (15, 15, 15), (0, 2)), ve.op((10, 10, 10), (20, 20, 20), (-5, -7)), ve.op((3, 2, 1), (17, 4, 9), (6, 1)), ve.op((16, 3, 2), (18, 3, 30), (2, 0)),
               ve.op((31, 31, 31), (31, 31, 31), (4, 4)), ve.op((16, 16, 0), (31, 31, 15), (0, 0))]
    else:
        a.LoadWorld(w, S)
    occ0 = a.WorldInfo()[2].copy()
    a.EditWorldCells(ops)
    b.LoadWorld(ve.apply_ops(w, ops), S)
    occ1 = _stores_agree(a, b, S, f"{form} store")
    assert form == "generated" or (occ0 != occ1).any(), form          # some chunk changed sides
    a.EditWorldCells([ve.op((0, 0, 0), tuple(d - 1 for d in w.shape[:3]), (0, 0))])          # one op over everything: every chunk empty
    assert not a.WorldInfo()[2].any() and not a.ReadWorldCells().any()
    a.close(); b.close()


@pytest.mark.parametrize("form", ["device", "host", "generated"])
def test_an_edited_store_equals_a_load_of_the_edited_cells(product_lib, form):
    _store_case(form)


def test_store_refusals(product_lib):
    L = abi.load_library()
    r = RaytraceRenderer(_anchor(), 32, 16)
    keep = []

    def call(rows, n=None):
        arr = np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 9)); keep.append(arr)
        return L.ycge_world_store_edit(r.ctx, arr.ctypes.data, len(arr) if n is None else n), L.ycge_last_error(r.ctx) or b""

    good = ve.op((0, 0, 0), (1, 1, 1), (5, 5))
    rc, err = call([good])
    assert rc == abi.YCGE_ERR_INVALID_ARG and b"no world store" in err
    w = ve.store_world()
    r.LoadWorld(w, ve.STORE_CHUNK)
    for rows, n, needle in (([good], -1, b"bad op array"), ([good], (1 << 20) + 1, b"bad op array"), ([good, ve.op((0, 0, 0), (0, 0, 0), (1, 1), grid=1)], None, b"op 1: grid_index 1"),
                            ([good, ve.op((0, 5, 0), (0, 4, 0), (1, 1))], None, b"op 1: lo 5 > hi 4 on axis 1"), ([good, ve.op((0, 0, 0), (40, 0, 0), (1, 1))], None, b"op 1: the box leaves the store")):
        rc, err = call(rows, n)
        assert rc == abi.YCGE_ERR_INVALID_ARG and needle in err, (rc, err)
        _same(r.ReadWorldCells(), w, f"after {needle}")
    assert L.ycge_world_store_edit(r.ctx, None, 1) == abi.YCGE_ERR_INVALID_ARG and L.ycge_world_store_edit(r.ctx, None, 0) == abi.YCGE_OK
    world = abi.World(16, 2, 11, abi.Vec3(0, 0, 0), abi.Vec3(1, 1, 1))
    r.GenerateWorldStore(world, 2, 2, form="fields")
    rc, err = call([good])
    assert rc == abi.YCGE_ERR_UNSUPPORTED and b"a fields store holds no cells" in err and b"YCGE_WORLD_STORE_CELLS" in err, (rc, err)
    r.close()


# ------------------------------------------------------------------------------------------------ 6. edit_resident
def test_edit_resident_keeps_grids_and_store_in_step(product_lib, tmp_path):
    w, ops, S = ve.store_world(), ve.store_ops(), ve.STORE_CHUNK
    r = RaytraceRenderer(_anchor(), 32, 16)
    keep = []
    proto = _store_proto(keep)
    r.LoadWorld(w, S)
    loaded = {}
    keys, idx = world_file.load_all_resident(r, proto, (0.0, 0.0, 0.0), loaded)
    assert loaded[(2, 1, 2)] == -1 and loaded[(1, 0, 1)] >= 0
    info, attached = world_file.edit_resident(r, ops, loaded, S, proto=proto)
    assert attached == [(2, 1, 2)] and loaded[(2, 1, 2)] >= 0 and info["cells_changed"] > 0
    after = ve.apply_ops(w, ops)
    for key, i in sorted(loaded.items()):
        if i < 0:
            continue
        shape = tuple(min(S, w.shape[k] - key[k] * S) for k in range(3))
        rec, mats = r.read_grid(i, shape)
        want = after[key[0] * S:key[0] * S + shape[0], key[1] * S:key[1] * S + shape[1], key[2] * S:key[2] * S + shape[2]]
        _same(mats, ve.materials_of(want), f"chunk {key}: the edited resident grid against the restatement")
        r._check(r.L.ycge_scene_detach_grids(r.ctx, (C.c_int32 * 1)(i), 1))
        j = r.AttachWorldChunks([key], proto)[0]
        if j < 0:
            assert (mats < 0).all(), key          # the edit emptied it
            continue
        rec2, mats2 = r.read_grid(j, shape)
        _same(mats2, mats, f"chunk {key}: attached again from the edited store"); _same(_record_fields(rec2), _record_fields(rec), f"chunk {key}: record")
    world_file.save_resident(r, tmp_path / "saved.vg01", slab_planes=7)
    world_file.write_vg01(tmp_path / "want.vg01", after)
    assert (tmp_path / "saved.vg01").read_bytes() == (tmp_path / "want.vg01").read_bytes()
    r.close()


# ------------------------------------------------------------------------------------------------ 7. two device contexts
def test_edits_on_a_context_that_drives_two_devices(product_lib):
    _edit_against_attach(["13 x 9 x 21", "a chunk of the world"], ["attached", "uploaded"], devices=[0, 0])
    _store_case("device", devices=[0, 0])
    # the second device's copies took the edit too: the frames of the two-device context equal the one-device context's
    def run(devices):
        scene, world = _world_scene()
        loaded = {}
        _tick(scene, world, loaded, None, *PATH[0])
        r = RaytraceRenderer(flatten(scene), 160, 90, 60.0, 1, capture_debug=True, count_work=True, devices=devices)
        p = _pose(20.0, 3.0)
        r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        r.TryFlipAndBlit()
        info, reinstall = _edit_world(r, loaded, loaded, [ve.op((60, 30, 40), (75, 127, 60), (0, 0))])
        assert info["objects_installed"] == int(reinstall)
        r.TryFlipAndBlit()
        out = [r.read(b) for b in DEBUG_BUFFERS + (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY, abi.BUF_G_DEPTH)]
        r.close()
        return out, info

    (one, i1), (two, i2) = run(None), run([0, 0])
    assert i1 == i2 and i1["cells_changed"] > 1000
    for k, (a, b) in enumerate(zip(one, two)):
        _same(a, b, f"two devices: buffer {k}")
