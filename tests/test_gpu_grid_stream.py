"""-m gpu: chunk streaming - ycge_scene_attach_grids / ycge_scene_detach_grids (csrc/ycge_grid_encode.*; reference VolumeScene.Update ->
WorldManager.LoadChunksAround, Scenes/VolumeScenes.cs:63-64, WorldManager.cs:289-370).  Every comparison is bit for bit
(parity_util.mismatch_count == 0): the device encoder against the host encoder of ycge_scene_upload, a streamed context against a twin
that uploads the equivalent scene every tick and against the oracle, queries, frames in flight, refusals, two device contexts."""
import ctypes as C

import numpy as np
import pytest

import parity_util as pu
from yetanotherconsolegameengine_amd import abi, build, scenes, world_file
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import AmbientLight, Material, PointLight, Scene, Sphere, VolumeGrid, ZERO, flatten, grid_record, vec3

pytestmark = pytest.mark.gpu

CHUNK, VIEW = 32, 1
WORLD_MIN, VOXEL = (-48.0, 0.0, -48.0), (1.0, 1.0, 1.0)
# a walk of the small world that crosses chunk borders in x, in z and diagonally, and comes back: 14 ticks, 9 of which change the set
PATH = [(0.0, 0.0), (10.0, 0.0), (20.0, 3.0), (40.0, 3.0), (40.0, 20.0), (40.0, 40.0), (5.0, 5.0), (-20.0, -20.0), (-20.0, 10.0), (-20.0, 40.0),
        (5.0, 5.0), (40.0, 40.0), (40.0, 3.0), (0.0, 0.0)]
FRAME_BUFFERS = (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY, abi.BUF_PREV_NORMAL,
                 abi.BUF_PREV_DEPTH, abi.BUF_PREV_SKY, abi.BUF_DENOISED)
DEBUG_BUFFERS = (abi.BUF_RAYS, abi.BUF_PRIM_ID, abi.BUF_SUB_ID, abi.BUF_HIT_T, abi.BUF_RNG_STATE)
COUNTERS = ("n_rays", "n_box", "n_tri", "n_prim", "n_vox", "n_rays_dark")


def _world_scene(t01=0.5):
    """The small config-5 world's lights and sky with no chunk attached yet, and the preloaded world."""
    world = scenes.make_voxel_world(96, 128, 96)
    s = Scene()
    s.IsVolumeScene = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.0)
    lights, top, bottom = scenes.sun_moon_lights(t01)
    s.Lights.extend(lights)
    s.BackgroundTop, s.BackgroundBottom = top, bottom
    return s, world


def _tick(scene, world, loaded, x, z):
    return world_file.stream_view(scene, world, (x, 70.0, z), WORLD_MIN, VOXEL, CHUNK, VIEW, scenes.VoxelMaterialLookup, loaded)


def _pose(x, z):
    return dict(pos=(float(x), 70.0, float(z)), yaw=0.4, pitch=-0.45, fov=60.0)


def _same(a, b, label):
    assert a.shape == b.shape, label
    n = pu.mismatch_count(a, b)
    assert n == 0, f"{label}: {n} elements differ"


def _same_buffers(g, t, buffers, label):
    for which in buffers:
        _same(g.read(which), t.read(which), f"{label}: buffer {which}")


# ------------------------------------------------------------------------------------------------ 1. encoder against encoder
def _drawn_grids():
    rng = np.random.default_rng(17)
    mats = [Material(vec3(*rng.uniform(0.1, 0.9, 3)), 0.1, 0.0, ZERO) for _ in range(300)]

    def cells(shape, fill=0.5, pairs=6, metas=3):
        c = np.zeros(shape + (2,), np.int32)
        solid = rng.random(shape) < fill
        ids = rng.integers(1, pairs + 1, shape)
        c[..., 0] = np.where(solid, ids, rng.integers(-2, 1, shape))          # air: matId <= 0 ...
        c[..., 1] = rng.integers(0, metas, shape)                              # ... with any meta
        return c

    def grid(c, lookup=None, corner=(0.0, 0.0, 0.0), voxel=(1.0, 1.0, 1.0), **kw):
        lk = lookup if lookup is not None else (lambda a, b: mats[(a * 7 + b) % len(mats)])
        return VolumeGrid(c, vec3(*corner), vec3(*voxel), lk, **kw)

    out = {}
    out["sides that are no multiple of 8"] = grid(cells((13, 9, 21)), corner=(1.5, -2.0, 3.25), voxel=(0.5, 0.75, 1.25))
    out["1 x 1 x 1"] = grid(np.array([[[[3, 1]]]], np.int32))
    out["all air"] = grid(np.zeros((9, 8, 7, 2), np.int32))
    c = np.zeros((16, 16, 16, 2), np.int32); c[15, 15, 15] = (2, 1)
    out["one solid voxel in a corner"] = grid(c)
    out["more than 64 bricks"] = grid(cells((40, 33, 47), fill=0.2), EnableWireframe=False, WireWidthFraction=0.7, WireMaxDistance=-1.0)
    out["a chunk of the world"] = VolumeGrid(np.ascontiguousarray(scenes.make_voxel_world(96, 128, 96)[32:64, 32:64, 32:64]), vec3(-16, 32, -16), vec3(1, 1, 1),
                                             lambda a, b: mats[(a * 7 + b) % len(mats)])
    return mats, out


def _record_fields(rec):
    """the GGrid record with cell_offset (word 12) and lut_offset (word 16) blanked"""
    w = rec.view(np.uint32).copy()
    w[12] = 0; w[16] = 0
    return w


def _upload_and_attach(grids_records_fn, grid_shape, mats, lib=None):
    """The same ycge_grid once inside a ycge_scene_upload and once attached to a scene without it: (record, materials) of each."""
    anchor = Scene()
    for m in mats:
        anchor.Add(Sphere(vec3(0, -50, 0), 0.1, m))          # every material is a material of the upload
    fa = flatten(anchor)
    keep = []
    rec = grids_records_fn(lambda m: fa._mat_index[id(m)], keep)
    # inside an upload: the anchor's tables with one more grid
    sc = abi.Scene()
    C.memmove(C.byref(sc), C.byref(fa.struct), C.sizeof(sc))
    arr = (abi.Grid * 1)(rec)
    sc.grids, sc.n_grids = C.cast(arr, C.POINTER(abi.Grid)), 1
    up = RaytraceRenderer(None, 32, 16, lib=lib)
    up._check(up.L.ycge_scene_upload(up.ctx, C.byref(sc)))
    at = RaytraceRenderer(fa, 32, 16, lib=lib)
    out = (C.c_int32 * 1)(-7)
    at._check(at.L.ycge_scene_attach_grids(at.ctx, arr, 1, out))
    assert out[0] == 0
    a, b = up.read_grid(0, grid_shape), at.read_grid(0, grid_shape)
    st = at.grid_pool_stats()
    up.close(); at.close()
    return a, b, st


def test_device_encoder_equals_the_host_encoder_on_drawn_grids(product_lib):
    mats, grids = _drawn_grids()
    for label, vg in grids.items():
        (ra, ma), (rb, mb), st = _upload_and_attach(lambda mat_id, keep: grid_record(vg, mat_id, keep), vg.Cells.shape[:3], mats)
        assert st["device_encodes"] == 1 and st["host_encodes"] == 0, (label, st)
        _same(ma, mb, f"{label}: per-voxel materials")
        _same(_record_fields(ra), _record_fields(rb), f"{label}: record")
        assert ((ma >= 0) == (vg.Cells[..., 0] > 0)).all(), label


def test_default_material_misses_and_large_lookup_tables(product_lib):
    """Misses that fall to default_material (device), and a lookup table of more than 254 entries (the host encoder serves the attach)."""
    mats, _ = _drawn_grids()
    rng = np.random.default_rng(3)
    c = np.zeros((24, 17, 30, 2), np.int32)
    c[..., 0] = rng.integers(-1, 9, c.shape[:3]); c[..., 1] = rng.integers(0, 4, c.shape[:3])

    def partial(n_entries, default):
        def make(mat_id, keep):
            vg = VolumeGrid(c, vec3(0, 0, 0), vec3(1, 1, 1), lambda a, b: mats[(a * 5 + b) % 200])
            g = grid_record(vg, mat_id, keep)
            if n_entries <= g.n_lookup:
                g.n_lookup = n_entries                      # the rest of the pairs miss
            else:                                           # pad with entries no cell uses
                lut = (abi.VoxelLookup * n_entries)()
                for i in range(n_entries):
                    src = g.lookup[i] if i < g.n_lookup else None
                    lut[i].mat_id, lut[i].meta_id, lut[i].material = (src.mat_id, src.meta_id, src.material) if src else (1000 + i, 0, mat_id(mats[i % 200]))
                keep.append(lut)
                g.lookup, g.n_lookup = C.cast(lut, C.POINTER(abi.VoxelLookup)), n_entries
            g.default_material = default
            return g
        return make

    (ra, ma), (rb, mb), st = _upload_and_attach(partial(5, 7), c.shape[:3], mats)
    assert st["device_encodes"] == 1
    _same(ma, mb, "misses to default_material"); _same(_record_fields(ra), _record_fields(rb), "misses: record")
    assert (ma == 7).any()
    # exactly 255 distinct pairs, 254 of them in the lookup table: the device encoder takes it (one pair falls to default_material)
    keep_c = c
    c = np.zeros((32, 32, 32, 2), np.int32)
    c[..., 0] = 1 + (np.arange(32 ** 3).reshape(32, 32, 32) % 255); c[..., 1] = 5
    (ra, ma), (rb, mb), st = _upload_and_attach(partial(254, 3), c.shape[:3], mats)
    assert st["device_encodes"] == 1 and st["host_encodes"] == 0
    _same(ma, mb, "exactly 255 pairs"); _same(_record_fields(ra), _record_fields(rb), "exactly 255 pairs: record")
    assert (ma >= 0).all()
    c = keep_c
    (ra, ma), (rb, mb), st = _upload_and_attach(partial(300, -1), c.shape[:3], mats)
    assert st["host_encodes"] == 1 and st["device_encodes"] == 0
    _same(ma, mb, "n_lookup > 254"); _same(_record_fields(ra), _record_fields(rb), "n_lookup > 254: record")


# ------------------------------------------------------------------------------------------------ 2. streamed / uploading twin / oracle
@pytest.mark.parametrize("counting", [True, False], ids=["counting", "timed"])
def test_streamed_world_equals_the_uploading_twin_and_the_oracle(product_lib, oracle, counting):
    scene, world = _world_scene()
    loaded = {}
    x0, z0 = PATH[0]
    _tick(scene, world, loaded, x0, z0)
    # the first upload holds the first view only: the arena is packed full, so the first chunk that enters grows it; the return trip
    # finds the slots the walk gave back
    first = [o for o in scene.Objects]
    scene.Objects[:] = first[:len(first) // 2]
    for k in [k for k, v in loaded.items() if not any(v is o for o in scene.Objects)]:
        del loaded[k]
    W, H = 128, 72
    kw = dict(capture_debug=counting, count_work=counting)
    g = RaytraceRenderer(flatten(scene), W, H, 60.0, 1, **kw)
    t = RaytraceRenderer(flatten(scene), W, H, 60.0, 1, **kw)
    o = oracle.OracleRenderer(scene, W, H, 1, _pose(x0, z0)) if counting else None
    changed = 0
    for tick, (x, z) in enumerate(PATH):
        added, removed = _tick(scene, world, loaded, x, z)
        changed += bool(added or removed)
        g.StreamObjects(scene)
        eq = flatten(scene)                                  # the equivalent scene: same materials, same Objects, the grids they refer to
        t.UploadScene(eq)
        if o is not None:
            assert o.L.orc_scene_upload(o.ctx, eq.byref()) == 0
        p = _pose(x, z)
        for r in (g, t):
            r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        if o is not None:
            o.set_camera(p["pos"], p["yaw"], p["pitch"], p["fov"])
        for f in range(2):
            label = f"tick {tick} frame {f}"
            sg, stw = g.TryFlipAndBlit(want_sdr=True), t.TryFlipAndBlit(want_sdr=True)
            _same(sg, stw, f"{label}: SDR frame")
            _same_buffers(g, t, FRAME_BUFFERS + (DEBUG_BUFFERS if counting else ()), label)
            if counting:
                for k in COUNTERS:
                    assert getattr(g.stats, k) == getattr(t.stats, k), (label, k)
                o.render(stages=1, threads=16)
                st = pu.compare_frame(o, g)
                for k in ("rays", "prim_id", "sub_id", "hit_t", "rng_state", "sky", "g_depth", "current_hdr", "taa_history", "g_albedo", "g_normal"):
                    assert st[k + "_mismatch"] == 0, f"{label}: {k} differs from the oracle in {st[k + '_mismatch']} elements"
                for k in ("n_rays", "n_box", "n_tri", "n_prim", "n_vox"):
                    assert st[k][0] == st[k][1], f"{label}: counter {k} {st[k]}"
            else:
                assert g.timed_steps() == t.timed_steps(), label
    st = g.grid_pool_stats()
    print("pool after the walk:", st)
    assert len(PATH) >= 12 and changed >= 6, changed
    assert st["slots_reused"] >= 1 and st["arena_growths"] >= 1, st          # a walk that did neither proves nothing
    assert st["resident"] == sum(isinstance(ob, VolumeGrid) for ob in scene.Objects)
    g.close(); t.close()
    if o is not None:
        o.close()


def test_cached_chunks_stay_resident_and_change_nothing(product_lib):
    """keep_cached=True (the reference's chunk cache): chunks that left Scene.Objects stay resident and unreferenced.  Frames, the
    timed kernels' steps and - on the counting instances - the counters equal the twin that uploads the equivalent scene, also when no
    VolumeGrid is left in Scene.Objects at all (the kernel instantiation follows the objects, not the resident set)."""
    for counting in (True, False):
        scene, world = _world_scene()
        loaded = {}
        _tick(scene, world, loaded, *PATH[0])
        kw = dict(capture_debug=counting, count_work=counting)
        ball = Sphere(vec3(0.0, 60.0, -20.0), 6.0, scenes.VoxelMaterialLookup(1, 0))
        scene.Add(ball)
        g = RaytraceRenderer(flatten(scene), 128, 72, 60.0, 1, **kw)
        t = RaytraceRenderer(flatten(scene), 128, 72, 60.0, 1, **kw)
        p = _pose(0.0, 0.0)
        for r in (g, t):
            r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        resident0 = g.grid_pool_stats()["resident"]
        grids = [o for o in scene.Objects if isinstance(o, VolumeGrid)]
        for step, objects in enumerate(([ball] + grids[: len(grids) // 2], [ball], [ball] + grids)):
            scene.Objects[:] = objects
            g.StreamObjects(scene, keep_cached=True)
            t.UploadScene(flatten(scene))
            for f in range(2):
                label = f"cached, step {step} frame {f} ({'counting' if counting else 'timed'})"
                _same(g.TryFlipAndBlit(want_sdr=True), t.TryFlipAndBlit(want_sdr=True), f"{label}: SDR frame")
                _same_buffers(g, t, FRAME_BUFFERS + (DEBUG_BUFFERS if counting else ()), label)
                if counting:
                    for k in COUNTERS:
                        assert getattr(g.stats, k) == getattr(t.stats, k), (label, k)
                else:
                    assert g.timed_steps() == t.timed_steps(), label
            st = g.grid_pool_stats()
            assert st["resident"] == resident0 and st["device_encodes"] == 0, (step, st)          # nothing left, nothing was encoded again
        g.close(); t.close()


# ------------------------------------------------------------------------------------------------ 3. from nothing
def test_a_cornell_box_receives_grids(product_lib, oracle):
    box, w, h, ss, pose = scenes.config_scene(1)
    pal = [scenes.VoxelMaterialLookup(m, k) for m in range(1, 12) for k in range(3)]
    for m in {id(p): p for p in pal}.values():
        box.Add(Sphere(vec3(0, -40, 0), 0.01, m))            # the palette's materials are materials of the upload
    g = RaytraceRenderer(flatten(box), w, h, pose["fov"], ss, capture_debug=True, count_work=True)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    g.TryFlipAndBlit()
    assert g.grid_pool_stats()["arena_capacity"] == 0
    rng = np.random.default_rng(5)
    for k in range(3):
        c = np.zeros((9, 7, 11, 2), np.int32)
        c[..., 0] = rng.integers(0, 6, c.shape[:3])
        box.Add(VolumeGrid(c, vec3(-0.6 + 0.45 * k, 0.8, -2.0), vec3(0.04, 0.04, 0.04), scenes.VoxelMaterialLookup))
    g.StreamObjects(box)
    eq = flatten(box)
    t = RaytraceRenderer(eq, w, h, pose["fov"], ss, capture_debug=True, count_work=True)
    t.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    t.set_frame_counter(1)
    o = oracle.OracleRenderer(box, w, h, ss, pose, flat=eq)
    o.set_frame_counter(1)
    g.TryFlipAndBlit(); t.TryFlipAndBlit(); o.render(stages=1, threads=8)
    for which in DEBUG_BUFFERS + (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK):
        _same(g.read(which), t.read(which), f"box + grids: buffer {which}")
        _same(g.read(which), o.read(which), f"box + grids against the oracle: buffer {which}")
    for k in COUNTERS:
        assert getattr(g.stats, k) == getattr(t.stats, k), k
    assert g.stats.n_vox > 0          # the grids are walked
    g.close(); t.close(); o.close()


# ------------------------------------------------------------------------------------------------ 4. queries
def test_queries_after_a_tick_equal_the_oracle(product_lib, oracle):
    scene, world = _world_scene()
    loaded = {}
    _tick(scene, world, loaded, *PATH[0])
    g = RaytraceRenderer(flatten(scene), 64, 36, 60.0, 1)
    _tick(scene, world, loaded, 40.0, 40.0)
    g.StreamObjects(scene)
    o = oracle.OracleRenderer(scene, 64, 36, 1, _pose(40.0, 40.0))
    rng = np.random.default_rng(12)
    n = 4096
    org = rng.uniform((-60, 20, -60), (60, 120, 60), (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 2, 1] = -np.abs(d[: n // 2, 1]) - 0.3           # half of them look down at the world
    hits, ids = g.Hit(org, d)
    occ = g.Occluded(org, d)
    L = o.L
    L.orc_scene_hit_many.restype = C.c_int
    L.orc_scene_hit_many.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p]
    od = np.ascontiguousarray(np.concatenate([org, d], axis=1))
    tq = np.zeros(n, np.float32); pq = np.zeros(n, np.int32)
    assert L.orc_scene_hit_many(o.ctx, od.ctypes.data_as(C.POINTER(C.c_float)), n, 0.001, float(np.float32(3.4028234663852886e38)),
                                tq.ctypes.data_as(C.POINTER(C.c_float)), pq.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert (pq >= 0).sum() > n // 8
    assert pu.mismatch_count(pq, ids[:, 0]) == 0
    hit = pq >= 0
    assert pu.mismatch_count(tq[hit], hits[hit, 0]) == 0
    assert pu.mismatch_count(occ, hit) == 0
    g.close(); o.close()


# ------------------------------------------------------------------------------------------------ 5. in flight
def test_a_tick_between_frames_in_flight(product_lib):
    watch = (abi.BUF_CURRENT_HDR, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY)

    def run(in_flight):
        scene, world = _world_scene()
        loaded = {}
        _tick(scene, world, loaded, *PATH[0])
        r = RaytraceRenderer(flatten(scene), 160, 90, 60.0, 1)
        p = _pose(20.0, 3.0)
        r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        out = []
        for step in range(4):
            if step == 2:
                _tick(scene, world, loaded, 40.0, 40.0)
                r.StreamObjects(scene)
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


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_scene_alone(torch_hip_first):
    L = abi.load_library(build.build_variant("faultinject"))
    L.ycge_debug_fail_allocation.restype = C.c_int
    L.ycge_debug_fail_allocation.argtypes = [C.c_int64]
    scene, world = _world_scene()
    loaded = {}
    _tick(scene, world, loaded, *PATH[0])
    flat = flatten(scene)
    p = _pose(0.0, 0.0)
    empty = RaytraceRenderer(None, 64, 36, 60.0, 1, lib=L)
    out = (C.c_int32 * 2)(-7, -7)
    vg = VolumeGrid(np.ascontiguousarray(world[0:32, 32:64, 0:32]), vec3(-100, 32, -100), vec3(1, 1, 1), scenes.VoxelMaterialLookup)
    keep = []
    good = grid_record(vg, lambda m: flat._mat_index[id(m)], keep)
    assert L.ycge_scene_attach_grids(empty.ctx, (abi.Grid * 1)(good), 1, out) == abi.YCGE_ERR_NO_SCENE
    assert L.ycge_scene_detach_grids(empty.ctx, (C.c_int32 * 1)(0), 1) == abi.YCGE_ERR_NO_SCENE
    empty.close()

    g = RaytraceRenderer(flat, 64, 36, 60.0, 1, lib=L)
    twin = RaytraceRenderer(flat, 64, 36, 60.0, 1, lib=L)
    for r in (g, twin):
        r.SetCamera(p["pos"], p["yaw"], p["pitch"])
    n_up = flat.struct.n_grids

    def refused(call, status, label):
        before = g.grid_pool_stats()
        out[0] = out[1] = -7
        rc = call()
        assert rc == status, (label, rc, L.ycge_last_error(g.ctx))
        assert (out[0], out[1]) == (-7, -7), label
        after = g.grid_pool_stats()
        assert {k: v for k, v in after.items() if not k.startswith("last_")} == {k: v for k, v in before.items() if not k.startswith("last_")}, label
        g.TryFlipAndBlit(); twin.TryFlipAndBlit()
        _same_buffers(g, twin, (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY, abi.BUF_G_DEPTH), label)

    def variant(**kw):
        r = abi.Grid()
        C.memmove(C.byref(r), C.byref(good), C.sizeof(r))
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    assert L.ycge_scene_attach_grids(g.ctx, None, 0, None) == abi.YCGE_OK
    assert L.ycge_scene_detach_grids(g.ctx, None, 0) == abi.YCGE_OK
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, None, 1, out), abi.YCGE_ERR_INVALID_ARG, "null grids")
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(good), -1, out), abi.YCGE_ERR_INVALID_ARG, "negative n")
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 2)(good, variant(nx=0)), 2, out), abi.YCGE_ERR_INVALID_ARG, "an empty grid second in the batch")
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(variant(nx=1 << 15, ny=1 << 15, nz=2)), 1, out), abi.YCGE_ERR_UNSUPPORTED, "2^30 cells or more")
    bad_lut = (abi.VoxelLookup * 1)(); bad_lut[0].mat_id, bad_lut[0].meta_id, bad_lut[0].material = 1, 0, 10 ** 6
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(variant(lookup=C.cast(bad_lut, C.POINTER(abi.VoxelLookup)), n_lookup=1)), 1, out),
            abi.YCGE_ERR_INVALID_ARG, "a lookup entry with a material out of range")
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(variant(nx=1, ny=23170, nz=23170)), 1, out), abi.YCGE_ERR_UNSUPPORTED, "2^23 bricks across one face")
    assert b"2^23 bricks" in L.ycge_last_error(g.ctx)
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 2)(good, variant(n_lookup=1)), 2, out), abi.YCGE_ERR_INVALID_ARG, "a pair with no material")
    assert b"no material" in L.ycge_last_error(g.ctx)
    # the message names the LOWEST offending cell in `cells` order, whichever workgroup meets it: two pairs miss, far apart
    two = np.zeros((40, 40, 40, 2), np.int32)
    two[..., 0] = 1
    two[3, 1, 2] = (77, 4)              # cell (3 * 40 + 1) * 40 + 2: the lower one
    two[37, 39, 38] = (55, 9)
    keep.append(two)
    one_entry = (abi.VoxelLookup * 1)(); one_entry[0].mat_id, one_entry[0].meta_id, one_entry[0].material = 1, 0, 0
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(variant(nx=40, ny=40, nz=40, cells=two.ctypes.data_as(C.POINTER(C.c_int32)),
                                                                           lookup=C.cast(one_entry, C.POINTER(abi.VoxelLookup)), n_lookup=1, default_material=-1)), 1, out),
            abi.YCGE_ERR_INVALID_ARG, "two pairs with no material")
    assert b"(matId 77, metaId 4)" in L.ycge_last_error(g.ctx), L.ycge_last_error(g.ctx)
    many = np.ones((16, 16, 2, 2), np.int32); many[..., 1] = np.arange(512).reshape(16, 16, 2)
    keep.append(many)
    refused(lambda: L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(variant(nx=16, ny=16, nz=2, cells=many.ctypes.data_as(C.POINTER(C.c_int32)), n_lookup=0, default_material=0)), 1, out),
            abi.YCGE_ERR_UNSUPPORTED, "more than 255 distinct pairs")
    refused(lambda: L.ycge_scene_detach_grids(g.ctx, (C.c_int32 * 1)(0), 1), abi.YCGE_ERR_INVALID_ARG, "detach of a grid Scene.Objects hold")
    refused(lambda: L.ycge_scene_detach_grids(g.ctx, (C.c_int32 * 1)(n_up), 1), abi.YCGE_ERR_INVALID_ARG, "detach of an index that is not resident")
    # one allocation failure walked through an attach of two grids: every call is YCGE_OK or YCGE_ERR_OUT_OF_MEMORY, and a failed one changes nothing
    failed, n = 0, 0
    while True:
        before = g.grid_pool_stats()
        out[0] = out[1] = -7
        L.ycge_debug_fail_allocation(n)
        rc = L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 2)(good, good), 2, out)
        left = L.ycge_debug_fail_allocation(-1)
        assert rc in (abi.YCGE_OK, abi.YCGE_ERR_OUT_OF_MEMORY), (n, rc, L.ycge_last_error(g.ctx))
        if rc == abi.YCGE_OK:
            assert left >= 0, n
            break
        failed += 1
        assert (out[0], out[1]) == (-7, -7), n
        after = g.grid_pool_stats()
        assert {k: v for k, v in after.items() if not k.startswith("last_")} == {k: v for k, v in before.items() if not k.startswith("last_")}, n
        g.TryFlipAndBlit(); twin.TryFlipAndBlit()
        _same_buffers(g, twin, (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY), f"allocation {n} failed")
        n += 1
    assert failed >= 5, failed
    assert (out[0], out[1]) == (n_up, n_up + 1)
    refused(lambda: L.ycge_scene_detach_grids(g.ctx, (C.c_int32 * 2)(n_up, n_up), 2), abi.YCGE_ERR_INVALID_ARG, "an index named twice")
    # detach, then attach: the freed index comes back (the lowest free one first)
    assert L.ycge_scene_detach_grids(g.ctx, (C.c_int32 * 1)(n_up), 1) == abi.YCGE_OK
    assert L.ycge_scene_attach_grids(g.ctx, (abi.Grid * 1)(good), 1, out) == abi.YCGE_OK and out[0] == n_up
    st = g.grid_pool_stats()
    assert st["slots_reused"] == 1 and st["resident"] == n_up + 2, st
    g.TryFlipAndBlit(); twin.TryFlipAndBlit()
    _same_buffers(g, twin, (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY), "grids nothing refers to change no pixel")
    g.close(); twin.close()


# ------------------------------------------------------------------------------------------------ 7. two device contexts
def test_a_tick_on_a_context_that_drives_two_devices(product_lib):
    def run(devices):
        scene, world = _world_scene()
        loaded = {}
        _tick(scene, world, loaded, *PATH[0])
        r = RaytraceRenderer(flatten(scene), 160, 90, 60.0, 1, capture_debug=True, count_work=True, devices=devices)
        p = _pose(40.0, 40.0)
        r.SetCamera(p["pos"], p["yaw"], p["pitch"])
        r.TryFlipAndBlit()
        _tick(scene, world, loaded, 40.0, 40.0)
        r.StreamObjects(scene)
        r.TryFlipAndBlit()
        out = [r.read(b) for b in DEBUG_BUFFERS + (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY, abi.BUF_G_DEPTH)]
        r.close()
        return out

    one, two = run(None), run([0, 0])
    # a peer context refuses both calls: it is driven by its root
    scene, world = _world_scene()
    _tick(scene, world, {}, *PATH[0])
    flat = flatten(scene)
    r = RaytraceRenderer(flat, 64, 36, 60.0, 1, devices=[0, 0])
    peer = C.c_void_p(r.L.ycge_debug_peer_context(r.ctx, 0))
    assert peer.value and not r.L.ycge_debug_peer_context(r.ctx, 1)
    keep, out = [], (C.c_int32 * 1)(-7)
    vg = VolumeGrid(np.ascontiguousarray(world[0:32, 32:64, 0:32]), vec3(-100, 32, -100), vec3(1, 1, 1), scenes.VoxelMaterialLookup)
    rec = (abi.Grid * 1)(grid_record(vg, lambda m: flat._mat_index[id(m)], keep))
    before = r.grid_pool_stats()
    assert r.L.ycge_scene_attach_grids(peer, rec, 1, out) == abi.YCGE_ERR_INVALID_ARG and out[0] == -7
    assert b"driven by their root" in r.L.ycge_last_error(peer)
    assert r.L.ycge_scene_detach_grids(peer, (C.c_int32 * 1)(0), 1) == abi.YCGE_ERR_INVALID_ARG
    assert r.grid_pool_stats() == before
    r.close()
    for k, (a, b) in enumerate(zip(one, two)):
        _same(a, b, f"two devices: buffer {k}")
