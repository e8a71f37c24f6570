"""-m gpu: a mesh's triangle BVH built ON THE DEVICE at ycge_scene_upload (csrc/ycge_mesh_bvh_build.hip, driven by csrc/ycge_mesh_bvh.cpp;
reference MeshBVH.cs:371-576).  The tree must be the host builder's byte for byte - ycge_host_build_mesh, which the CPU suite holds against
the oracle - whatever the mesh, however many of its nodes are wider than one workgroup (YCGE_MESH_BVH_WIDE_MIN drives that on small
meshes), and uploads through it must leave the oracle's trees and the oracle's frames."""
import ctypes as C
import time

import numpy as np
import pytest

import parity_util as pu
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import (AmbientLight, Box, Material, Mesh, PointLight, Scene, Solid, Sphere, flatten, vec3, ZERO)

pytestmark = pytest.mark.gpu
f32 = np.float32
NODE = np.dtype([("w", "<u4", 10)])          # a 40-byte reference node, compared as bytes


def _host_tree(L, tris):
    n = len(tris)
    L.ycge_host_build_mesh.restype = C.c_int
    L.ycge_host_build_mesh.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    t = np.ascontiguousarray(tris, dtype=f32).reshape(-1, 9)
    nodes = np.zeros(max(1, 2 * n), NODE); leaf = np.zeros(max(1, n), np.int32); st = np.zeros(3, np.int32)
    k = L.ycge_host_build_mesh(t.ctypes.data, n, nodes.ctypes.data, leaf.ctypes.data, st.ctypes.data)
    return k, nodes[:k], leaf[:n], int(st[1]), int(st[2])


def _device_tree(L, tris):
    n = len(tris)
    fn = L.ycge_debug_device_mesh_bvh
    fn.restype, fn.argtypes = abi.MESH_BVH_HOOK_PROTOTYPES["ycge_debug_device_mesh_bvh"]
    t = np.ascontiguousarray(tris, dtype=f32).reshape(-1, 9)
    nodes = np.zeros(max(1, 2 * n), NODE); leaf = np.zeros(max(1, n), np.int32); res = np.zeros(abi.MESH_BVH_RES_WORDS, np.uint32)
    k = fn(t.ctypes.data, n, nodes.ctypes.data, leaf.ctypes.data, res.ctypes.data)
    assert k >= 0, f"ycge_debug_device_mesh_bvh returned {k}"
    return k, nodes[:k], leaf[:n], res


def _same(L, tris, label):
    """the device builder's tree against the host builder's; returns (res16, host sorts)"""
    k, hn, hl, depth, sorts = _host_tree(L, tris)
    kd, dn, dl, res = _device_tree(L, tris)
    assert kd == k, f"{label}: {kd} nodes, host {k}"
    assert hn.tobytes() == dn.tobytes(), f"{label}: nodes differ"
    assert (hl == dl).all(), f"{label}: leaf order differs"
    assert int(res[0]) == depth and int(res[1]) == sorts, f"{label}: depth {res[0]} / sorts {res[1]}, host {depth} / {sorts}"
    return res, sorts


def _tris(centres, size, rng):
    """one small triangle about every centre"""
    c = np.asarray(centres, f32)
    off = rng.uniform(-1.0, 1.0, (len(c), 3, 3)).astype(f32) * np.broadcast_to(np.asarray(size, f32), (len(c),)).reshape(-1, 1, 1)
    return (c[:, None, :] + off).astype(f32)


def _wide_min(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("YCGE_MESH_BVH_WIDE_MIN", raising=False)
    else:
        monkeypatch.setenv("YCGE_MESH_BVH_WIDE_MIN", value)
    return 2560 if value is None else int(value)


WIDE = [pytest.param("9", id="wide9"), pytest.param("64", id="wide64"), pytest.param(None, id="default")]


@pytest.mark.parametrize("wide_min", WIDE)
def test_builder_alone_at_the_sizes_that_change_its_code_path(product_lib, monkeypatch, wide_min):
    """No triangle, a root that is a leaf (<= 8), one split, one / just over one 64-item chunk, the one-workgroup capacity and one more,
    several workgroups per node, several wide levels."""
    wm = _wide_min(monkeypatch, wide_min)
    rng = np.random.default_rng(31)
    for n in (0, 1, 8, 9, 16, 17, 64, 65, 2560, 2561, 6000, 20000):
        tris = _tris(rng.uniform(-20, 20, (n, 3)), 0.05, rng)
        res, _ = _same(product_lib, tris, f"uniform {n}")
        if n:
            assert res[5] == 1 and res[4] == abi.MESH_BVH_BUILT, f"uniform {n}: not built on the device ({res[4]})"
            assert (res[2] > 0) == (n > wm), f"uniform {n}: {res[2]} wide nodes with WIDE_MIN {wm}"
            assert res[3] >= 1


@pytest.mark.parametrize("wide_min", WIDE)
def test_builder_alone_on_hard_triangle_sets(product_lib, monkeypatch, wide_min):
    """Item sets chosen to hit the builder's ties and edge cases.  Array.Sort inside a subtree is built on the device; Array.Sort at a node
    wider than one workgroup, and a NaN, go to the host builder - the hook names the reason and still returns the host's tree.  (With
    WIDE_MIN 9 every node that could need Array.Sort - more than 8 items - IS wide, so there the 40 identical triangles fall back too.)"""
    wm = _wide_min(monkeypatch, wide_min)
    L = product_lib
    rng = np.random.default_rng(77)
    g = np.stack(np.meshgrid(np.arange(17), np.arange(11), np.arange(17), indexing="ij"), -1).reshape(-1, 3).astype(f32)       # 3 179
    lattice = g[:, None, :] * f32(2.0) + np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)[None]
    cases = {
        "uniform 3000": _tris(rng.uniform(-50, 50, (3000, 3)), 0.2, rng),
        "lattice of equal triangles": lattice,
        "lattice, shuffled": lattice[rng.permutation(len(lattice))],
        "centroids on a plane": _tris(np.c_[rng.uniform(-9, 9, 3000), np.full(3000, 2.5), rng.uniform(-9, 9, 3000)], 0.0, rng) + np.asarray([[0, 0, 0], [.1, 0, 0], [0, 0, .1]], f32),
        "centroids on a line": _tris(np.c_[np.linspace(-40, 40, 2999), np.zeros(2999), np.zeros(2999)], 0.0, rng) + np.asarray([[0, 0, 0], [.1, 0, 0], [.1, 0, 0]], f32),
        "clusters": _tris(np.repeat(rng.uniform(-30, 30, (12, 3)), 250, 0) + rng.normal(0, 0.05, (3000, 3)), 0.02, rng),
        "quantised to integers": np.round(_tris(rng.uniform(-1, 1, (3000, 3)), 0.6, rng)).astype(f32),
        "250 triangles, 12 times each": np.repeat(_tris(rng.uniform(-10, 10, (250, 3)), 0.3, rng), 12, 0)[rng.permutation(3000)],
        "signed zeros, sizes 1e-3 .. 1e6": _tris(np.where(rng.random((2800, 3)) < 0.3, -0.0, rng.uniform(-1, 1, (2800, 3))), rng.choice([1e-3, 1.0, 1e6], 2800), rng)
                                           * np.where(rng.random((2800, 3, 3)) < 0.1, f32(-0.0), f32(1.0)),
    }
    device_sorted = 0
    for label, tris in cases.items():
        res, sorts = _same(L, tris, label)
        if res[5] == 1:
            device_sorted += sorts > 0
        else:       # Array.Sort at a wide node is the one reason such a set may go to the host
            assert res[4] in (abi.MESH_BVH_SORT_NO_SPLIT, abi.MESH_BVH_SORT_EMPTY_SIDE), f"{label}: fallback {res[4]}"
            assert wm < 2560, f"{label}: fell back at the default WIDE_MIN"
    same40 = np.tile(f32([[[1, 2, 3], [2, 2, 3], [1, 3, 3]]]), (40, 1, 1))
    res, sorts = _same(L, same40, "40 identical triangles")
    assert sorts >= 1
    if wm >= 40:
        assert res[5] == 1 and res[4] == abi.MESH_BVH_BUILT and res[2] == 0
        device_sorted += 1
    else:
        assert res[5] == 0 and res[4] == abi.MESH_BVH_SORT_NO_SPLIT
    if wide_min is None:
        res, sorts = _same(L, np.tile(same40[:1], (5000, 1, 1)), "5 000 identical triangles")
        assert res[5] == 0 and res[4] == abi.MESH_BVH_SORT_NO_SPLIT and sorts >= 1
    nan = cases["uniform 3000"].copy()
    nan[1234, 1, 2] = np.nan
    res, _ = _same(L, nan, "a NaN vertex")
    assert res[5] == 0 and res[4] == abi.MESH_BVH_NON_FINITE
    print(f"WIDE_MIN {wm}: {len(cases) + 1} sets, {device_sorted} of them through Array.Sort on the device")
    if wm >= 40:
        assert device_sorted >= 2


# ---------------------------------------------------------------------------------- through ycge_scene_upload
def _same_mesh_trees(o, g, n_meshes, label):
    for mi in range(n_meshes):
        assert pu.bits_equal(o.accel(abi.ACCEL_MESH_NODES, mi), g.accel(abi.ACCEL_MESH_NODES, mi)), f"{label}: nodes of mesh {mi} differ"
        assert pu.bits_equal(o.accel(abi.ACCEL_MESH_LEAF_INDEX, mi), g.accel(abi.ACCEL_MESH_LEAF_INDEX, mi)), f"{label}: leaf order of mesh {mi} differs"


def _frame_parity(o, g, label):
    o.render(stages=1, threads=16); g.TryFlipAndBlit()
    st = pu.compare_frame(o, g)
    for k in ("rays", "prim_id", "sub_id", "hit_t", "rng_state", "sky", "g_depth", "current_hdr", "taa_history", "g_albedo", "g_normal"):
        assert st[k + "_mismatch"] == 0, f"{label}: {k} differs in {st[k + '_mismatch']} elements"
    for k in ("n_rays", "n_box", "n_tri", "n_prim", "n_vox"):
        assert st[k][0] == st[k][1], f"{label}: counter {k}"


def _live(L):
    out = (C.c_int64 * 6)()
    assert L.ycge_debug_live_resources(out) == abi.YCGE_OK
    return list(out)


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one device", "two devices"])
def test_config_3_uploaded_through_the_device_builder(product_lib, oracle, monkeypatch, devices):
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    sc, w, h, ss, pose = scenes.config_scene(3)
    flat = flatten(sc)
    o = oracle.OracleRenderer(sc, 160, 90, 1, pose, flat=flat)
    kw = dict(devices=devices) if devices else {}
    g = RaytraceRenderer(flat, 160, 90, pose["fov"], 1, capture_debug=True, count_work=True, **kw)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    _same_mesh_trees(o, g, 1, "config 3")
    _frame_parity(o, g, "config 3")
    st = g.mesh_bvh_stats()
    print("config 3:", st)
    assert st["device_builds"] == 1 and st["host_builds"] == 0 and st["host_fallbacks"] == 0 and st["wide_nodes"] >= 1 and st["subtree_workgroups"] >= 2
    if not devices:
        # a second upload on the same context: the same trees, and the builder's scratch is given back again
        live = _live(g.L)
        g._check(g.L.ycge_scene_upload(g.ctx, flat.byref()))
        _same_mesh_trees(o, g, 1, "config 3, second upload")
        assert g.mesh_bvh_stats()["device_builds"] == 2
        assert _live(g.L)[:2] == live[:2], (live, _live(g.L))
    o.close(); g.close()


def _two_mesh_scene():
    rng = np.random.default_rng(4)
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.3)
    m = [Material(vec3(*rng.uniform(0.2, 0.9, 3)), 0.1, 0.0, ZERO) for _ in range(3)]
    s.Add(Mesh(_tris(rng.uniform((-2.5, 0.2, -6), (-0.5, 2, -4), (9, 3)), 0.3, rng), m[0]))
    s.Add(Mesh(_tris(rng.uniform((0, 0.2, -7), (3, 2.5, -4), (3000, 3)), 0.06, rng), m[1]))
    s.Add(Sphere(vec3(-1.0, 0.5, -3.0), 0.5, m[2]))
    s.Add(Box(vec3(-6, -0.2, -9), vec3(6, 0.0, 0), Solid(vec3(0.6, 0.6, 0.6)), 0.1, 0.0))
    s.Lights.append(PointLight(vec3(0, 5, -2), vec3(1, 1, 1), 80.0))
    s.BackgroundTop, s.BackgroundBottom = vec3(0.5, 0.7, 1.0), vec3(0.9, 0.95, 1.0)
    return s, dict(pos=(0.0, 1.2, 1.0), yaw=0.0, pitch=-0.05, fov=55.0)


def test_the_builder_is_picked_per_mesh_by_triangle_count(product_lib, oracle, monkeypatch):
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1000")
    s, pose = _two_mesh_scene()
    o, g = pu.run_pair(oracle, s, 160, 90, 1, pose, frames=0)
    _same_mesh_trees(o, g, 2, "9 and 3 000 triangles")
    _frame_parity(o, g, "9 and 3 000 triangles")
    st = g.mesh_bvh_stats()
    assert st["device_builds"] == 1 and st["host_builds"] == 1 and st["host_fallbacks"] == 0, st
    o.close(); g.close()


def test_the_host_knob_keeps_every_mesh_on_the_host(product_lib, oracle, monkeypatch):
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    monkeypatch.setenv("YCGE_MESH_BVH_HOST", "1")
    s, pose = _two_mesh_scene()
    o, g = pu.run_pair(oracle, s, 96, 54, 1, pose, frames=0)
    _same_mesh_trees(o, g, 2, "host knob")
    st = g.mesh_bvh_stats()
    assert st["device_builds"] == 0 and st["host_builds"] == 2, st
    o.close(); g.close()


# ---------------------------------------------------------------------------------- full size, tree only
def test_config_4_mesh_tree_at_full_size(product_lib):
    """The one larger case: config 4's 871 200 triangles through the builder alone.  The two times are printed, never asserted."""
    sc = scenes.config_scene(4)[0]
    tris = next(ob.Triangles for ob in sc.Objects if isinstance(ob, Mesh))
    t0 = time.perf_counter(); k, hn, hl, depth, sorts = _host_tree(product_lib, tris); t_host = time.perf_counter() - t0
    t0 = time.perf_counter(); kd, dn, dl, res = _device_tree(product_lib, tris); t_dev = time.perf_counter() - t0
    print(f"config 4: {len(tris)} triangles, {k} nodes, depth {depth}; host builder {t_host * 1e3:.1f} ms, device hook {t_dev * 1e3:.1f} ms "
          f"(build alone {int(res[7])} us, {int(res[2])} wide nodes in {int(res[6])} levels, {int(res[3])} subtree workgroups)")
    assert res[5] == 1 and res[4] == abi.MESH_BVH_BUILT
    assert kd == k and hn.tobytes() == dn.tobytes() and (hl == dl).all() and int(res[0]) == depth and int(res[1]) == sorts
