"""-m gpu: Scene.Hit / Scene.Occluded as batched queries on the device scene (ycge_scene_hit / ycge_scene_occluded, ABI 10), against the
oracle bit for bit.

Every ray's hit flag is compared with the oracle's Scene.Hit; on hits the object index, the sub id and every float of the record
{t, P, N, albedo}.  Whole batches go through orc_scene_hit_many (t and object), full records through orc_scene_hit (>= 4 096 rays per case).
Both sides normalise the direction as `new Ray(o, d)` does (Ray.cs:8-12).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import parity_util as pu
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import (AmbientLight, Checker, Material, Mesh, Plane, PointLight, Scene, Sphere, VolumeGrid, flatten,
                                                   vec3)
from random_scenes import random_scene

pytestmark = pytest.mark.gpu

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)
INF = F32(np.inf)


# ---------------------------------------------------------------------------------------------------------------------------- helpers
def _bind_hit_many(ob):
    L = ob.lib()
    L.orc_scene_hit_many.restype = C.c_int
    L.orc_scene_hit_many.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float),
                                     C.POINTER(C.c_int32), C.c_void_p]
    return L


def oracle_many(ob, o, od, t_min, t_max):
    """(t, object) of n rays with one [t_min, t_max] (orc_scene_hit_many): t = t_max and object -1 on a miss"""
    L = _bind_hit_many(ob)
    od = np.ascontiguousarray(od, dtype=F32)
    n = od.shape[0]
    t = np.zeros(n, F32); prim = np.zeros(n, np.int32)
    assert L.orc_scene_hit_many(o.ctx, od.ctypes.data_as(C.POINTER(C.c_float)), n, float(t_min), float(t_max),
                                t.ctypes.data_as(C.POINTER(C.c_float)), prim.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    return t, prim


def oracle_records(o, rays):
    """(flag[n], rec[n, 13]) from orc_scene_hit: {hit, object, sub, t, P, N, albedo} per ray (per-ray tmin / tmax)"""
    rec = np.zeros((rays.shape[0], 13), F32)
    for i, r in enumerate(rays):
        rec[i] = o.scene_hit(r[0:3], r[3:6], r[6], r[7])
    return rec[:, 0] != 0, rec


def assert_records_equal(rays, hits, ids, occl, flag, rec, what=""):
    """the product's records against the oracle's, bit for bit"""
    got = ids[:, 0] >= 0
    bad = np.nonzero(got != flag)[0]
    assert bad.size == 0, (what, "hit flag", bad[:8], rays[bad[:4]])
    if occl is not None:
        badb = np.nonzero(occl != flag)[0]
        assert badb.size == 0, (what, "occluded", badb[:8], rays[badb[:4]])
    h = np.nonzero(flag)[0]
    assert np.array_equal(ids[h, 0], rec[h, 1].astype(np.int32)), (what, "object")
    assert np.array_equal(ids[h, 1].astype(F32), rec[h, 2]), (what, "sub")            # (the oracle hands the sub id over as a float)
    assert pu.mismatch_count(hits[h], rec[h, 3:13]) == 0, (what, "record", h[np.nonzero((hits[h].view(np.uint32) != rec[h, 3:13].view(np.uint32)).any(axis=1))[0][:4]])
    m = np.nonzero(~flag)[0]
    assert (ids[m] == -1).all() and (hits[m] == 0).all(), (what, "miss record")


def query_and_compare(g, o, rays, what=""):
    hits, ids = g.Hit(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    occl = g.Occluded(rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    flag, rec = oracle_records(o, rays)
    assert_records_equal(rays, hits, ids, occl, flag, rec, what)
    return hits, ids, flag


def normalized(d):
    """Vec3.Normalized (Vec3.cs:98-107) in binary32"""
    d = d.astype(F32)
    l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inv = F32(1.0) / np.sqrt(l2)
    return np.where((l2 <= 0)[:, None], d, d * inv[:, None]).astype(F32)


def scene_box(g):
    """min / max of the scene tree's nodes, clipped to +-60 (planes are unbounded)"""
    nodes = g.accel(abi.ACCEL_SCENE_NODES)
    if nodes.size == 0:
        return np.full(3, -5, F32), np.full(3, 5, F32)
    lo = np.clip(nodes["min"].min(axis=0), -60, 60).astype(F32)
    hi = np.clip(nodes["max"].max(axis=0), -60, 60).astype(F32)
    return lo, np.maximum(hi, lo + F32(1.0))


def random_rays(seed, lo, hi, n=4096):
    """origins inside and around the bounds; direction lengths 1e-3 .. 1e3, axis-aligned directions, +-0 components; the drawn intervals.
    What these rays do not reach: drawn from a continuous distribution, no origin lies in the plane of a box (so a zero direction component
    never meets a 0 * inf slab product), no ray passes exactly through an edge, rim or vertex two primitives share, none ends on its hit to
    the ulp, no denominator lands beside its cut-off, no voxel walk ties.  Those rays are tests/seam_rays.py, held to the oracle by
    tests/test_gpu_seam_rays.py."""
    rng = np.random.default_rng(seed)
    ext = hi - lo
    o = (lo - 0.2 * ext + rng.random((n, 3)) * 1.4 * ext).astype(F32)
    d = rng.normal(size=(n, 3))
    d *= (10.0 ** rng.uniform(-3, 3, n))[:, None] / np.linalg.norm(d, axis=1)[:, None]
    d = d.astype(F32)
    ax = rng.random(n) < 0.15                               # axis-aligned: one component, the others +0 or -0
    k = rng.integers(0, 3, n)
    for i in np.nonzero(ax)[0]:
        v = np.where(rng.random(3) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
        v[k[i]] = F32(rng.choice([-1, 1]) * 10.0 ** rng.uniform(-3, 3))
        d[i] = v
    z = rng.random((n, 3)) < 0.05                           # stray signed zeros
    d[z & ~ax[:, None]] = F32(-0.0)
    tmin = rng.choice(np.array([0.0, 1e-5, 0.001, 0.5], F32), n)
    tmax = rng.choice(np.array([0.65, 10.0, FLT_MAX, INF], F32), n)
    inv = rng.random(n) < 0.05                              # tmin > tmax: a miss, as in the reference
    tmin[inv], tmax[inv] = F32(0.5), F32(0.25)
    rays = np.concatenate([o, d, tmin[:, None], tmax[:, None]], axis=1).astype(F32)
    lsq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return rays[np.isfinite(lsq) & (lsq > 0)]                  # (what the library refuses is test_refusals' business)


def shadow_rays(hits, ids, lights, n_max=4096):
    """from every hit point to each light, maxDist = the distance (Scene.Occluded(new Ray(p, toL), dist))"""
    p = hits[ids[:, 0] >= 0, 1:4][: max(1, n_max // max(1, len(lights)))]
    out = []
    for l in lights:
        to = (np.asarray(l.Position, F32)[None, :] - p).astype(F32)
        dist = np.sqrt((to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2]).astype(F32)
        keep = dist > 0
        r = np.zeros((int(keep.sum()), 8), F32)
        r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = p[keep], to[keep], F32(0.001), dist[keep]
        out.append(r)
    return np.concatenate(out) if out else np.zeros((0, 8), F32)


def frame_pair(ob, n, small_dims, t01=0.25):
    sc, _, _, _, pose = scenes.config_scene(n, small=(n == 5), t01=t01)
    w, h, ss = small_dims
    flat = flatten(sc)
    o = ob.OracleRenderer(sc, w, h, ss, pose, flat=flat)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss, capture_debug=True)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    g.SetFov(pose.get("fov", 45.0))
    g.TryFlipAndBlit()
    return sc, o, g


CONFIGS = [(1, (80, 45, 1), 0.25), (2, (160, 45, 1), 0.25), (3, (320, 90, 1), 0.25), (4, (320, 90, 1), 0.25), (5, (160, 45, 1), 0.25),
           (5, (160, 45, 1), 0.5)]
CONFIG_IDS = ["c1", "c2", "c3", "c4", "c5-dark", "c5-noon"]


# ------------------------------------------------------------------------------------------------------------- 1-4: configs 1-5
@pytest.mark.parametrize("n,dims,t01", CONFIGS, ids=CONFIG_IDS)
def test_configs_primary_random_and_shadow_rays(product_lib, oracle, n, dims, t01):
    sc, o, g = frame_pair(oracle, n, dims, t01)
    try:
        # 1. the frame's own primary rays (Ray.Dir as the frame traced it, tMin 0.001, tMax FLT_MAX)
        r6 = g.read(abi.BUF_RAYS).reshape(-1, 6)
        prim, sub, hit_t = g.read(abi.BUF_PRIM_ID).ravel(), g.read(abi.BUF_SUB_ID).ravel(), g.read(abi.BUF_HIT_T).ravel()
        rays = np.concatenate([r6, np.full((r6.shape[0], 1), 0.001, F32), np.full((r6.shape[0], 1), FLT_MAX, F32)], axis=1)
        hits, ids = g.Hit(rays[:, 0:3], rays[:, 3:6], F32(0.001), FLT_MAX)
        t_o, p_o = oracle_many(oracle, o, r6, F32(0.001), FLT_MAX)
        assert np.array_equal(ids[:, 0], p_o)
        h = p_o >= 0
        assert pu.mismatch_count(hits[h, 0], t_o[h]) == 0
        # Ray.Dir is already a unit vector; the query normalises it once more (new Ray(o, d)).  Where that leaves the direction's bits as
        # they were, the query IS the frame's primary query: same object, sub id and t as YCGE_BUF_PRIM_ID / SUB_ID / HIT_T
        same = (normalized(r6[:, 3:6]).view(np.uint32) == r6[:, 3:6].view(np.uint32)).all(axis=1)
        assert same.mean() > 0.3, same.mean()
        assert np.array_equal(ids[same, 0], prim[same])
        hs = same & (prim >= 0)
        assert np.array_equal(ids[hs, 1], sub[hs]) and pu.mismatch_count(hits[hs, 0], hit_t[hs]) == 0
        # full records on a subsample
        sel = np.random.default_rng(n).choice(rays.shape[0], min(4096, rays.shape[0]), replace=False)
        hits_p, ids_p, _ = query_and_compare(g, o, rays[sel], "primary")
        # 2. seeded random rays in and around the scene
        lo, hi = scene_box(g)
        query_and_compare(g, o, random_rays(1000 + n, lo, hi), "random")
        # 4. shadow rays towards each light from the primary hit points
        sh = shadow_rays(hits_p, ids_p, sc.Lights)
        if sh.shape[0]:
            query_and_compare(g, o, sh, "shadow")
    finally:
        o.close(); g.close()


def test_volume_scene_probe_shapes(product_lib, oracle):
    """3. VolumeScene's probes on the voxel world: the five-ray downward ground fan with tMin = 1e-5 (VolumeScenes.cs:477-528) and the
    collision capsule's horizontal rays with tMax = CollisionRadius = 0.65 (:215-260, :446), from points on and above the ground."""
    sc, o, g = frame_pair(oracle, 5, (160, 45, 1), 0.5)
    try:
        rng = np.random.default_rng(5)
        lo, hi = scene_box(g)
        n = 1024
        feet = (lo + rng.random((n, 3)) * (hi - lo)).astype(F32)
        feet[:, 1] = hi[1] + F32(2.0)
        down = np.zeros((n, 8), F32); down[:, 0:3] = feet; down[:, 4] = F32(-1.0); down[:, 6] = F32(1e-5); down[:, 7] = FLT_MAX
        hits, ids = g.Hit(down[:, 0:3], down[:, 3:6], down[:, 6], down[:, 7])
        ground = hits[ids[:, 0] >= 0, 1:4]
        assert ground.shape[0] > n // 4
        fan = []
        for dx, dz in ((0, 0), (0.3, 0), (-0.3, 0), (0, 0.3), (0, -0.3)):
            r = np.zeros((ground.shape[0], 8), F32)
            r[:, 0:3] = ground + np.array([dx, 1.6, dz], F32)
            r[:, 4] = F32(-1.0); r[:, 6] = F32(1e-5); r[:, 7] = F32(2.5)
            fan.append(r)
        query_and_compare(g, o, np.concatenate(fan)[:4096], "ground fan")
        caps = []
        for k in range(16):
            a = 2 * np.pi * k / 16
            for y in (0.2, 0.9, 1.6):
                r = np.zeros((ground.shape[0], 8), F32)
                r[:, 0:3] = ground + np.array([0, y, 0], F32)
                r[:, 3], r[:, 5] = F32(np.cos(a)), F32(np.sin(a))
                r[:, 6], r[:, 7] = F32(0.001), F32(0.65)
                caps.append(r)
        caps = np.concatenate(caps)
        query_and_compare(g, o, caps[np.random.default_rng(6).choice(caps.shape[0], 4096, replace=False)], "capsule")
    finally:
        o.close(); g.close()


# ------------------------------------------------------------------------------------------------------------- 5: drawn scenes, object lists
@pytest.mark.parametrize("seed", range(8))
def test_drawn_scenes(product_lib, oracle, seed):
    s, pose = random_scene(700 + seed)
    flat = flatten(s)
    o = oracle.OracleRenderer(s, 48, 16, 1, pose, flat=flat)
    g = RaytraceRenderer(flat, 48, 16, pose.get("fov", 45.0), 1)
    try:
        lo, hi = scene_box(g)
        rays = random_rays(seed, lo, hi)
        hits, ids, _ = query_and_compare(g, o, rays, f"seed {seed}")
        sh = shadow_rays(hits, ids, s.Lights)
        if sh.shape[0]:
            query_and_compare(g, o, sh, f"seed {seed} shadow")
    finally:
        o.close(); g.close()


def test_object_lists_installed_by_update_objects(product_lib, oracle):
    """the empty list (all misses), analytic objects only, a grid world with its walk tree, up to four objects (one leaf) and a real tree;
    the oracle gets the same flat scene"""
    floor = Plane(vec3(0, 0, 0), vec3(0, 1, 0), Checker(vec3(0.8, 0.8, 0.8), vec3(0.2, 0.2, 0.2), 1.0), 0.0, 0.0)
    ball = Sphere(vec3(-1.2, 0.7, -3.0), 0.7, Material(vec3(0.95, 0.95, 0.95), 0.0, 0.95))
    pos, faces = scenes.make_torus_knot(24, 8)
    mesh = Mesh((pos[faces] * np.float32(0.35) + np.float32([0.8, 0.9, -3.2])).astype(np.float32), Material(vec3(0.2, 0.7, 0.3), 0.1, 0.0))

    def grid(corner, seed):
        r_ = np.random.default_rng(seed)
        cells = np.zeros((6, 6, 6, 2), np.int32)
        cells[..., 0] = np.where(r_.random((6, 6, 6)) < 0.5, r_.integers(1, 12, (6, 6, 6)), 0)
        return VolumeGrid(cells, corner, vec3(0.3, 0.3, 0.3), scenes.VoxelMaterialLookup, True, 0.06, 16.0)

    g1, g2 = grid(vec3(-0.4, 0.0, -2.2), 1), grid(vec3(1.6, 0.0, -4.5), 2)
    universe = [floor, ball, mesh, g1, g2]
    s = Scene()
    s.Objects = list(universe)
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Lights.append(PointLight(vec3(1.0, 4.0, 0.0), vec3(1, 1, 1), 50.0))
    pose = dict(pos=(0.2, 1.1, 0.8), yaw=0.05, pitch=-0.15, fov=55.0)
    uploaded = flatten(s)
    o = oracle.OracleRenderer(s, 32, 9, 1, pose, flat=uploaded)
    g = RaytraceRenderer(uploaded, 32, 9, pose["fov"], 1)
    lists = [[], [floor], [ball, floor], [g1], [g1, g2], [mesh], [floor, mesh, g1], [g1, g2, mesh, floor], universe, universe[::-1],
             universe + universe, [g1, g2, g1, g2, mesh], [floor] * 5, [mesh] * 5]
    lists += [list(c_) for c_ in itertools.islice(itertools.product(universe, repeat=3), 0, 125, 9)]
    lo, hi = np.array([-3, -0.5, -6], F32), np.array([3, 3, 1], F32)
    try:
        for k, li in enumerate(lists):
            s.Objects = li
            f = flatten(s, against=uploaded)
            assert o.L.orc_scene_upload(o.ctx, f.byref()) == 0
            g.UpdateObjects(f)
            rays = random_rays(50 + k, lo, hi, n=4096)
            _, ids, _ = query_and_compare(g, o, rays, f"list {k}")
            if not li:
                assert (ids[:, 0] == -1).all()
    finally:
        o.close(); g.close()


# ------------------------------------------------------------------------------------------------------------- 6: batch sizes
def test_batch_sizes(product_lib, oracle):
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    o = oracle.OracleRenderer(sc, w, h, ss, pose, flat=flat)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss)
    try:
        rng = np.random.default_rng(3)
        big = 1 << 20                                          # larger than the resident lanes of any MI355X grid (256 CUs x 16 x 64)
        o_ = (np.array([-1.0, 0.2, -1.0]) + rng.random((big, 3)) * np.array([2.0, 1.6, 2.0])).astype(F32)
        d_ = rng.normal(size=(big, 3)).astype(F32)
        for n in (1, 63, 64, 65, 4096):
            r = np.concatenate([o_[:n], d_[:n], np.full((n, 1), 0.001, F32), np.full((n, 1), FLT_MAX, F32)], axis=1)
            query_and_compare(g, o, r, f"n = {n}")
        hits, ids = g.Hit(np.zeros((0, 3), F32), np.zeros((0, 3), F32))
        assert hits.shape == (0, 10) and ids.shape == (0, 2)
        assert g.Occluded(np.zeros((0, 3), F32), np.zeros((0, 3), F32)).shape == (0,)
        hits, ids = g.Hit(o_, d_, F32(0.001), FLT_MAX)
        occl = g.Occluded(o_, d_, F32(0.001), FLT_MAX)
        t_o, p_o = oracle_many(oracle, o, np.concatenate([o_, d_], axis=1), F32(0.001), FLT_MAX)
        assert np.array_equal(ids[:, 0], p_o) and np.array_equal(occl, p_o >= 0)
        hm = p_o >= 0
        assert pu.mismatch_count(hits[hm, 0], t_o[hm]) == 0
        assert hm.mean() > 0.5
    finally:
        o.close(); g.close()


# ------------------------------------------------------------------------------------------------------------- 7: frames unaffected
def _probe(g, k):
    rng = np.random.default_rng(k)
    o = (rng.random((200, 3)) * 2 - 1).astype(F32)
    d = rng.normal(size=(200, 3)).astype(F32)
    g.Hit(o, d)
    g.Occluded(o, d, F32(0.0), F32(0.65))


POSES = [((0.0, 1.0, 0.0), 0.0, 0.0), ((0.0, 1.0, 0.0), 0.0, 0.0), ((0.05, 1.0, 0.1), 0.02, -0.01), ((0.05, 1.0, 0.1), 0.02, -0.01)]


def test_frames_unaffected_synchronous(product_lib):
    """the same frames, bit for bit - SDR, TAA history, RNG state - with queries between them and without"""
    sc, w, h, ss, pose = scenes.config_scene(2)
    flat = flatten(sc)
    out = []
    for with_queries in (False, True):
        g = RaytraceRenderer(flat, 160, 45, 45.0, 1, capture_debug=True)
        frames = []
        for k, (p, y, pt) in enumerate(POSES):
            g.SetCamera(p, y, pt)
            if with_queries: _probe(g, k)
            sdr = g.TryFlipAndBlit(want_sdr=True)
            if with_queries: _probe(g, 10 + k)
            frames.append((sdr, g.read(abi.BUF_TAA_HISTORY), g.read(abi.BUF_RNG_STATE), int(g.stats.frame)))
        out.append(frames)
        g.close()
    for a, b in zip(*out):
        assert pu.mismatch_count(a[0], b[0]) == 0 and pu.mismatch_count(a[1], b[1]) == 0 and np.array_equal(a[2], b[2]) and a[3] == b[3]


@pytest.mark.parametrize("n", [2, 5])
def test_frames_unaffected_in_flight(product_lib, n):
    """frames in flight (FrameLate's ycge_render_frame_async_sdr): a query between two of them does not join the one in flight -
    frames_outstanding stays 1 - and the frames are the ones the same sequence without queries gives"""
    sc, w, h, ss, pose = scenes.config_scene(n, small=(n == 5), t01=0.5)
    flat = flatten(sc)
    p0 = pose["pos"]
    out = []
    for with_queries in (False, True):
        g = RaytraceRenderer(flat, 160, 45, pose.get("fov", 45.0), 1)
        sdrs = []
        for k in range(4):
            g.SetCamera((p0[0] + 0.01 * k, p0[1], p0[2]), pose["yaw"], pose["pitch"])
            a = g.RenderAsync(sdr_slot=k % 2)
            if with_queries:
                _probe(g, k)
                assert g.flight_info()["frames_outstanding"] == 1
            g.Wait()
            sdrs.append(a.copy())
        out.append((sdrs, g.read(abi.BUF_TAA_HISTORY)))
        g.close()
    for a, b in zip(out[0][0], out[1][0]):
        assert pu.mismatch_count(a, b) == 0
    assert pu.mismatch_count(out[0][1], out[1][1]) == 0


# ------------------------------------------------------------------------------------------------------------- 8: refusals
def test_refusals(product_lib, oracle):
    L = product_lib
    g0 = RaytraceRenderer(None, 16, 8, 45.0, 1)
    try:
        with pytest.raises(abi.YcgeError) as e:
            g0.Hit(np.zeros((1, 3), F32), np.ones((1, 3), F32))
        assert e.value.status == abi.YCGE_ERR_NO_SCENE
        with pytest.raises(abi.YcgeError) as e:
            g0.Occluded(np.zeros((1, 3), F32), np.ones((1, 3), F32))
        assert e.value.status == abi.YCGE_ERR_NO_SCENE
    finally:
        g0.close()
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    o = oracle.OracleRenderer(sc, w, h, ss, pose, flat=flat)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss)
    try:
        rng = np.random.default_rng(8)
        good = np.concatenate([(rng.random((100, 3)) - 0.5).astype(F32), rng.normal(size=(100, 3)).astype(F32),
                               np.full((100, 1), 0.001, F32), np.full((100, 1), FLT_MAX, F32)], axis=1)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        hits = np.zeros((100, 10), F32); ids = np.zeros((100, 2), np.int32); occ = np.zeros(100, np.uint8)
        ip = ids.ctypes.data_as(C.POINTER(C.c_int32)); up = occ.ctypes.data_as(C.POINTER(C.c_uint8))
        assert L.ycge_scene_hit(None, fp(good), 1, fp(hits), ip) == abi.YCGE_ERR_INVALID_ARG
        assert L.ycge_scene_occluded(None, fp(good), 1, up) == abi.YCGE_ERR_INVALID_ARG
        for args in ((fp(good), -1, fp(hits), ip), (None, 1, fp(hits), ip), (fp(good), 1, None, ip), (fp(good), 1, fp(hits), None)):
            assert L.ycge_scene_hit(g.ctx, *args) == abi.YCGE_ERR_INVALID_ARG
        for args in ((fp(good), -1, up), (None, 1, up), (fp(good), 1, None)):
            assert L.ycge_scene_occluded(g.ctx, *args) == abi.YCGE_ERR_INVALID_ARG
        assert L.ycge_scene_hit(g.ctx, None, 0, None, None) == abi.YCGE_OK and L.ycge_scene_occluded(g.ctx, None, 0, None) == abi.YCGE_OK
        nan, inf = F32(np.nan), F32(np.inf)
        cases = [(0, nan, "origin"), (1, inf, "origin"), (2, -inf, "origin"), (3, nan, "direction"), (4, inf, "direction"), (6, nan, "tmin"),
                 (6, inf, "tmin"), (6, -inf, "tmin"), (7, nan, "tmax")]
        bad_dirs = [np.zeros(3, F32), np.array([-0.0, 0.0, -0.0], F32), np.array([1e20, 0, 0], F32), np.array([1e-23, 0, 0], F32)]
        for k, (col, v, word) in enumerate(cases + [(None, d, "normalis") for d in bad_dirs]):
            r = good.copy()
            j = 17 + 3 * k
            if col is None: r[j, 3:6] = v
            else: r[j, col] = v
            r[j + 5, 0] = nan                                   # (a later bad ray: the first one is named)
            for fn, args in ((L.ycge_scene_hit, (fp(r), 100, fp(hits), ip)), (L.ycge_scene_occluded, (fp(r), 100, up))):
                assert fn(g.ctx, *args) == abi.YCGE_ERR_INVALID_ARG, (k, fn)
                msg = L.ycge_last_error(g.ctx).decode()
                assert f"ray {j}:" in msg and word in msg, (k, msg)
            query_and_compare(g, o, good, f"after refusal {k}")           # the context is usable and right
        ok = good.copy(); ok[:, 7] = inf                                   # accepted: tmax = +inf, FLT_MAX, tmin > tmax
        ok[:10, 6], ok[:10, 7] = F32(2.0), F32(1.0)
        query_and_compare(g, o, ok, "accepted")
    finally:
        o.close(); g.close()


# ------------------------------------------------------------------------------------------------------------- 9: other contexts
def test_multi_device_root_and_resident_rank(product_lib, oracle):
    sc, w, h, ss, pose = scenes.config_scene(2)
    flat = flatten(sc)
    o = oracle.OracleRenderer(sc, 64, 18, 1, pose, flat=flat)
    lo, hi = np.array([-4, -0.5, -8], F32), np.array([4, 3, 1], F32)
    rays = random_rays(9, lo, hi)
    try:
        root = RaytraceRenderer(flat, 64, 18, pose.get("fov", 45.0), 1, devices=[0, 0, 0])      # three contexts on one GPU: the root answers
        try:
            root.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
            root.TryFlipAndBlit()
            query_and_compare(root, o, rays, "root")
            root.TryFlipAndBlit()
        finally:
            root.close()
        rank = RaytraceRenderer(flat, 64, 18, pose.get("fov", 45.0), 1, rank=1, world_size=2, tile_ring=2)     # its own full copy of the scene
        try:
            query_and_compare(rank, o, rays, "tile-resident rank")
        finally:
            rank.close()
    finally:
        o.close()


# ------------------------------------------------------------------------------------------------------------- 10: fault injection
def test_allocation_failure_in_the_first_query(product_lib, oracle):
    """lib/var_faultinject.so: the n-th host allocation of the first query fails -> YCGE_ERR_OUT_OF_MEMORY, and the context still answers"""
    from yetanotherconsolegameengine_amd import build
    L = abi.load_library(build.build_variant("faultinject"))
    L.ycge_debug_fail_allocation.restype = C.c_int
    L.ycge_debug_fail_allocation.argtypes = [C.c_int64]
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    o = oracle.OracleRenderer(sc, w, h, ss, pose, flat=flat)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss, lib=L)
    rays = random_rays(10, np.array([-1, 0, -1], F32), np.array([1, 2, 1], F32), n=512)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    try:
        failed, n = 0, 0
        while True:
            hits = np.zeros((rays.shape[0], 10), F32); ids = np.zeros((rays.shape[0], 2), np.int32)
            L.ycge_debug_fail_allocation(n)
            rc = L.ycge_scene_hit(g.ctx, fp(rays), rays.shape[0], fp(hits), ids.ctypes.data_as(C.POINTER(C.c_int32)))
            left = L.ycge_debug_fail_allocation(-1)
            if rc == abi.YCGE_ERR_OUT_OF_MEMORY:
                failed += 1
                assert b"bad_alloc" in L.ycge_last_error(g.ctx)
            else:
                assert rc == abi.YCGE_OK, (n, rc)
                flag, rec = oracle_records(o, rays)
                assert_records_equal(rays, hits, ids, None, flag, rec, f"n = {n}")
                if left >= 0: break
            n += 1
        assert failed >= 1
        query_and_compare(g, o, rays, "after")
    finally:
        o.close(); g.close()
