"""-m gpu: the mesh arena assembled ON THE DEVICE at ycge_scene_upload (csrc/ycge_mesh_emit.hip, driven by csrc/ycge_mesh_bvh.cpp): the GNode /
GTriPair records of every mesh and the cooperative walk's treelet region, byte for byte what emit_mesh_records and append_treelets write on
the host.  ycge_debug_device_mesh_arena is the twin of ycge_host_mesh_arena_treelets (one mesh, no context); whole uploads are compared
through ycge_debug_read_mesh_arena with the same upload under YCGE_MESH_EMIT_HOST=1, and rendered against the oracle."""
import ctypes as C

import numpy as np
import pytest

import parity_util as pu
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import AmbientLight, Box, Material, Mesh, PointLight, Scene, Solid, flatten, vec3, ZERO

pytestmark = pytest.mark.gpu
f32 = np.float32
NODE = np.dtype([("mn", "<f4", 3), ("mx", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("start", "<i4"), ("count", "<i4")])
REF_NONE = 0xffffffff


def _t9(tris):
    return np.ascontiguousarray(tris, dtype=f32).reshape(-1, 9)


def _host(L, tris):
    """(bytes, root_ref, tl_offset) as the host lays one mesh out"""
    t = _t9(tris)
    fn = L.ycge_host_mesh_arena_treelets
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    root, tl = C.c_uint32(0), C.c_uint32(0)
    n = fn(t.ctypes.data, len(t), None, 0, C.byref(root), C.byref(tl))
    assert n >= 0, n
    out = np.zeros(max(n, 1), np.uint8)
    assert fn(t.ctypes.data, len(t), out.ctypes.data, n, C.byref(root), C.byref(tl)) == n
    return out[:n], int(root.value), int(tl.value)


def _device(L, tris, capacity):
    t = _t9(tris)
    fn = L.ycge_debug_device_mesh_arena
    fn.restype, fn.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_device_mesh_arena"]
    root, tl = C.c_uint32(0x12345678), C.c_uint32(0x12345678)
    out = np.full(capacity + 4096, 0xa5, np.uint8)          # (a stale byte the kernels leave behind would show)
    res = np.zeros(abi.MESH_EMIT_RES_WORDS, np.uint32)
    n = fn(t.ctypes.data, len(t), out.ctypes.data, out.nbytes, C.byref(root), C.byref(tl), res.ctypes.data)
    assert n >= 0, f"ycge_debug_device_mesh_arena returned {n}"
    assert n <= capacity and (out[n:] == 0xa5).all()
    return out[:n], int(root.value), int(tl.value), dict(zip(abi.MESH_EMIT_RES, (int(v) for v in res)))


def _same(L, tris, label):
    """the device's arena of one mesh against the host's: size, root reference, treelet offset, every byte"""
    hb, hroot, htl = _host(L, tris)
    db, droot, dtl, res = _device(L, tris, len(hb))
    assert len(db) == len(hb), f"{label}: {len(db)} bytes, host {len(hb)}"
    assert droot == hroot, f"{label}: root {droot:#x}, host {hroot:#x}"
    assert dtl == htl, f"{label}: treelets at {dtl}, host {htl}"
    if not np.array_equal(db, hb):
        at = int(np.flatnonzero(db != hb)[0])
        raise AssertionError(f"{label}: {int((db != hb).sum())} bytes differ, the first at {at} (records end at {htl or len(hb)})")
    return res, hb, hroot, htl


def _tris(centres, size, rng):
    c = np.asarray(centres, f32)
    off = rng.uniform(-1.0, 1.0, (len(c), 3, 3)).astype(f32) * np.broadcast_to(np.asarray(size, f32), (len(c),)).reshape(-1, 1, 1)
    return (c[:, None, :] + off).astype(f32)


def _uniform(n, seed=31):
    rng = np.random.default_rng(seed)
    return _tris(rng.uniform(-20, 20, (n, 3)), 0.05, rng)


def _host_nodes(L, tris):
    t = _t9(tris)
    L.ycge_host_build_mesh.restype = C.c_int
    L.ycge_host_build_mesh.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    nodes = np.zeros(max(1, 2 * len(t)), NODE); leaf = np.zeros(max(1, len(t)), np.int32); st = np.zeros(3, np.int32)
    k = L.ycge_host_build_mesh(t.ctypes.data, len(t), nodes.ctypes.data, leaf.ctypes.data, st.ctypes.data)
    return nodes[:k]


def _internal_levels(nodes):
    """levels of internal nodes below (and with) the root: 0 for a leaf root"""
    deepest, todo = 0, [(0, 1)]
    while todo:
        i, d = todo.pop()
        if nodes["count"][i] > 0: continue
        deepest = max(deepest, d)
        todo += [(int(nodes["left"][i]), d + 1), (int(nodes["right"][i]), d + 1)]
    return deepest


def _wide_min(monkeypatch, value):
    if value is None: monkeypatch.delenv("YCGE_MESH_BVH_WIDE_MIN", raising=False)
    else: monkeypatch.setenv("YCGE_MESH_BVH_WIDE_MIN", value)


# ---------------------------------------------------------------------------------- one mesh, the kernels against the host's bytes
def test_no_triangle_and_roots_that_are_leaves(product_lib):
    """n = 0: no records, REF_NONE.  n = 1, 2, 3, 8: the root is a leaf, no treelets; an odd leaf's last slot is all zeros."""
    res, hb, root, tl = _same(product_lib, np.zeros((0, 3, 3), f32), "no triangle")
    assert len(hb) == 0 and root == REF_NONE and tl == 0
    for n in (1, 2, 3, 8):
        res, hb, root, tl = _same(product_lib, _uniform(n), f"{n} triangles")
        assert root >> 29 == 3 and (root & 15) == n and tl == 0 and len(hb) == 96 * ((n + 1) // 2)
        assert res["nodes"] == 1 and res["record_units"] == 3 * ((n + 1) // 2)
        if n & 1:
            slot1 = hb[-96:].view(np.uint32).reshape(12, 2)[:, 1]
            assert (slot1 == 0).all()


def test_a_node_over_two_leaves(product_lib):
    """n = 9, 16, 17: the root is a node; over two leaves (9 always: a leaf holds 8) its treelet has depth 1 - slots 0 and 1, twelve of zeros."""
    for n in (9, 16, 17):
        res, hb, root, tl = _same(product_lib, _uniform(n), f"{n} triangles")
        levels = _internal_levels(_host_nodes(product_lib, _uniform(n)))
        assert levels >= 1 and (levels == 1 or n != 9)
        assert root >> 29 == 2 and tl != 0 and tl % 512 == 0
        slots = hb[tl: tl + 14 * 32].view(np.uint32).reshape(14, 8)
        assert (slots[:2, 7] == 1).all()
        if levels == 1:
            assert res["nodes"] == 3 and (slots[2:] == 0).all()


def test_treelets_of_trees_of_two_three_and_four_levels(product_lib):
    """The treelet's cut at depth 3: trees of exactly 2, 3 and 4 levels of internal nodes (the sizes are found on the host, the depth asserted)."""
    L = product_lib
    base = _uniform(400, seed=5)
    found = {}
    for n in range(17, 400):
        d = _internal_levels(_host_nodes(L, base[:n]))
        if d in (2, 3, 4) and d not in found: found[d] = n
        if len(found) == 3: break
    assert sorted(found) == [2, 3, 4], found
    for d, n in sorted(found.items()):
        assert _internal_levels(_host_nodes(L, base[:n])) == d
        res, hb, root, tl = _same(L, base[:n], f"{n} triangles, {d} levels of nodes")
        slots = hb[tl: tl + 14 * 32].view(np.uint32).reshape(14, 8)          # the root's treelet (unit 0)
        assert slots[:2, 7].all() and slots[2:6, 7].any() == (d >= 2) and slots[6:, 7].any() == (d >= 3)


def test_the_treelet_region_starts_on_512_bytes_either_way(product_lib):
    """One size whose record bytes are a multiple of 512 (t0 = the records' end) and one whose are not (a zeroed gap in front of t0)."""
    L = product_lib
    base = _uniform(600, seed=9)
    L.ycge_host_mesh_arena.restype = C.c_int
    L.ycge_host_mesh_arena.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    root = C.c_uint32(0)
    aligned = ragged = None
    for n in range(20, 600):
        nbytes = L.ycge_host_mesh_arena(_t9(base[:n]).ctypes.data, n, None, 0, C.byref(root))
        if nbytes % 512 == 0 and aligned is None: aligned = (n, nbytes)
        if nbytes % 512 != 0 and ragged is None: ragged = (n, nbytes)
        if aligned and ragged: break
    assert aligned and ragged, (aligned, ragged)
    for (n, nbytes), gap in ((aligned, False), (ragged, True)):
        res, hb, root_ref, tl = _same(L, base[:n], f"{n} triangles, {nbytes} bytes of records")
        assert res["record_units"] * 32 == nbytes and tl == (nbytes + 511) // 512 * 512 and (tl > nbytes) == gap
        assert (hb[nbytes:tl] == 0).all() and len(hb) == tl + res["record_units"] * 256


@pytest.mark.parametrize("wide_min", [pytest.param("9", id="wide9"), pytest.param(None, id="default")])
def test_hard_sets_and_trees_of_several_wide_levels(product_lib, monkeypatch, wide_min):
    """The hard sets of test_gpu_mesh_bvh_device_build.py: coincident triangles (Array.Sort at a wide node: the host's tree goes through the
    device emit), slivers in a line (a deep chain), a non-finite coordinate (host tree; the NaN travels through the subtractions) - and plain
    sizes around the builder's thresholds, with YCGE_MESH_BVH_WIDE_MIN at 9 (every node above a leaf is wide) and unset."""
    _wide_min(monkeypatch, wide_min)
    L = product_lib
    rng = np.random.default_rng(77)
    same40 = np.tile(f32([[[1, 2, 3], [2, 2, 3], [1, 3, 3]]]), (40, 1, 1))
    uniform = _tris(rng.uniform(-50, 50, (3000, 3)), 0.2, rng)
    nan = uniform.copy()
    nan[1234, 1, 2] = np.nan
    res, *_ = _same(L, same40, "40 identical triangles")
    assert res["tree_built_on_device"] == (0 if wide_min == "9" else 1)
    if wide_min is None:          # Array.Sort at a node wider than one workgroup: the host's tree
        res, *_ = _same(L, np.tile(same40[:1], (5000, 1, 1)), "5 000 identical triangles")
        assert res["tree_built_on_device"] == 0
    line = _tris(np.c_[np.linspace(-40, 40, 2999), np.zeros(2999), np.zeros(2999)], 0.0, rng) + np.asarray([[0, 0, 0], [.1, 0, 0], [.1, 0, 0]], f32)
    _same(L, line, "slivers in a line")
    res, *_ = _same(L, nan, "a NaN vertex")
    assert res["tree_built_on_device"] == 0
    for n in (65, 2560, 2561, 6000):
        res, *_ = _same(L, _uniform(n), f"uniform {n}")
        assert res["tree_built_on_device"] == 1


def test_the_bunny(product_lib):
    """The committed bunny (69 451 triangles): units above 2^16, several scan tiles."""
    tris = scenes.BuildBunnyScene().Objects[1].Triangles
    assert len(tris) == 69451
    res, hb, root, tl = _same(product_lib, tris, "the bunny")
    print("the bunny:", res, len(hb), "bytes")
    assert res["tree_built_on_device"] == 1 and res["record_units"] > 1 << 16 and res["nodes"] > 4 * 1024


# ---------------------------------------------------------------------------------- whole uploads
def _four_mesh_flat(bad_material=False):
    """Meshes of 1, 0, 500 (a material per triangle) and 3 000 triangles; the empty one is in the mesh table only (an object without
    bounds is refused by Scene.Objects' builder, on either path)."""
    rng = np.random.default_rng(4)
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.3)
    m = [Material(vec3(*rng.uniform(0.2, 0.9, 3)), 0.1, 0.0, ZERO) for _ in range(5)]
    s.Add(Mesh(_tris([(-2.0, 1.0, -5.0)], 0.4, rng), m[0]))
    s.Add(Mesh(np.zeros((0, 3, 3), f32), m[0]))
    s.Add(Mesh(_tris(rng.uniform((-2.5, 0.2, -6), (-0.5, 2, -4), (500, 3)), 0.1, rng), m[1], TriMaterials=m[1:4], TriMaterialIndex=rng.integers(0, 3, 500)))
    s.Add(Mesh(_tris(rng.uniform((0, 0.2, -7), (3, 2.5, -4), (3000, 3)), 0.06, rng), m[4]))
    s.Add(Box(vec3(-6, -0.2, -9), vec3(6, 0.0, 0), Solid(vec3(0.6, 0.6, 0.6)), 0.1, 0.0))
    s.Lights.append(PointLight(vec3(0, 5, -2), vec3(1, 1, 1), 80.0))
    s.BackgroundTop, s.BackgroundBottom = vec3(0.5, 0.7, 1.0), vec3(0.9, 0.95, 1.0)
    flat = flatten(s)
    n = flat.struct.n_prims
    assert flat.prims[1].type == abi.PRIM_MESH and flat.prims[1].ref == 1 and flat.meshes[1].n_triangles == 0
    keep = [flat.prims[i] for i in range(n) if i != 1]
    arr = (abi.Prim * len(keep))(*keep)
    flat._keep.append(arr)
    flat.prims = arr
    flat.struct.prims, flat.struct.n_prims = C.cast(arr, C.POINTER(abi.Prim)), len(keep)
    if bad_material:
        flat.meshes[2].tri_material[137] = flat.struct.n_materials
    return flat


def _upload(flat, monkeypatch, emit_host, env=()):
    monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", "1")          # (the default is the measured crossover: these meshes are below it)
    for k, v in env: monkeypatch.setenv(k, v)
    if emit_host: monkeypatch.setenv("YCGE_MESH_EMIT_HOST", "1")
    else: monkeypatch.delenv("YCGE_MESH_EMIT_HOST", raising=False)
    g = RaytraceRenderer(flat, 64, 36, 55.0, 1)          # (the knobs are read once, at ycge_create)
    arena, tl = g.read_mesh_arena()
    out = (arena.copy(), tl, g.read_meshes().copy(), g.mesh_emit_stats(), g.mesh_bvh_stats())
    g.close()
    return out


def _same_arena(d, h, label):
    """two uploads (_upload's tuples) hold the same arena: size, treelet offset, GMesh records, every byte"""
    (da, dtl, dm, dst, _), (ha, htl, hm, hst, _) = d, h
    assert dst["arena_bytes"] == hst["arena_bytes"] == len(ha) == len(da), (label, dst, hst)
    assert dtl == htl, f"{label}: treelets at {dtl}, host {htl}"
    assert np.array_equal(dm, hm), f"{label}: GMesh records differ"
    assert np.array_equal(da, ha), f"{label}: {int((da != ha).sum())} bytes of the arena differ, the first at {int(np.flatnonzero(da != ha)[0])}"


def _same_upload(flat, monkeypatch, env, label):
    d, h = _upload(flat, monkeypatch, False, env), _upload(flat, monkeypatch, True, env)
    (da, dtl, dm, dst, dbvh), hst = d, h[3]
    assert hst["device_meshes"] == 0 and hst["host_meshes"] == 4 and hst["last_device_emit_us"] == 0, hst
    assert dst["device_meshes"] == 4 and dst["host_meshes"] == 0, dst
    _same_arena(d, h, label)
    return da, dtl, dm, dbvh


def test_four_meshes_in_one_arena(product_lib, monkeypatch):
    flat = _four_mesh_flat()
    arena, tl, meshes, bvh = _same_upload(flat, monkeypatch, (("YCGE_MESH_BVH_DEVICE_MIN", "1"),), "four meshes")
    assert bvh["device_builds"] == 3 and bvh["host_builds"] == 1          # (the empty mesh is no build of the device's)
    roots = meshes[:, 6]
    assert roots[0] >> 29 == 3 and roots[1] == REF_NONE and roots[2] >> 29 == 2 and roots[3] >> 29 == 2
    units = (roots & 0x1ffffff0) >> 4
    assert units[0] == 0 and units[2] == 3 and units[3] > units[2] and tl != 0          # base units: non-zero from the second mesh on


def test_host_built_and_device_built_trees_in_one_device_arena(product_lib, monkeypatch):
    flat = _four_mesh_flat()
    arena, tl, meshes, bvh = _same_upload(flat, monkeypatch, (("YCGE_MESH_BVH_DEVICE_MIN", "1000"),), "DEVICE_MIN 1000")
    assert bvh["device_builds"] == 1 and bvh["host_builds"] == 3, bvh


def _declined_flat(with_a_built_mesh):
    """Mesh 0: 40 identical triangles, which the device builder declines under YCGE_MESH_BVH_WIDE_MIN=9 (Array.Sort at a wide node:
    MESH_BVH_SORT_NO_SPLIT, test_gpu_mesh_bvh_device_build.py); mesh 1, on request: 500 drawn triangles, which it builds."""
    rng = np.random.default_rng(4)
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.3)
    same40 = np.tile(f32([[[1, 2, 3], [2, 2, 3], [1, 3, 3]]]), (40, 1, 1))
    s.Add(Mesh(same40, Material(vec3(0.8, 0.3, 0.2), 0.1, 0.0, ZERO)))
    if with_a_built_mesh:
        s.Add(Mesh(_tris(rng.uniform((-2.5, 0.2, -6), (-0.5, 2, -4), (500, 3)), 0.1, rng), Material(vec3(0.2, 0.5, 0.8), 0.1, 0.0, ZERO)))
    s.Add(Box(vec3(-6, -0.2, -9), vec3(6, 0.0, 0), Solid(vec3(0.6, 0.6, 0.6)), 0.1, 0.0))
    s.Lights.append(PointLight(vec3(0, 5, -2), vec3(1, 1, 1), 80.0))
    s.BackgroundTop, s.BackgroundBottom = vec3(0.5, 0.7, 1.0), vec3(0.9, 0.95, 1.0)
    return flatten(s), same40


DECLINING = (("YCGE_MESH_BVH_DEVICE_MIN", "1"), ("YCGE_MESH_BVH_WIDE_MIN", "9"))


def test_a_tree_the_builder_declined_in_a_device_made_arena(product_lib, monkeypatch):
    """The builder declines mesh 0 inside an upload and builds mesh 1: the host's tree of mesh 0 is uploaded and joins the arena the
    device writes (mesh_emit_add, built = false) - the bytes of the same upload under YCGE_MESH_EMIT_HOST=1."""
    flat, _ = _declined_flat(True)
    d, h = _upload(flat, monkeypatch, False, DECLINING), _upload(flat, monkeypatch, True, DECLINING)
    print("device emit:", d[3], d[4], "host emit:", h[3], h[4])
    assert d[4]["device_builds"] == 1 and d[4]["host_fallbacks"] == 1, d[4]
    assert d[3]["device_meshes"] == 2 and d[3]["host_meshes"] == 0, d[3]
    assert h[3]["device_meshes"] == 0 and h[3]["host_meshes"] == 2 and h[3]["last_device_emit_us"] == 0, h[3]
    _same_arena(d, h, "a declined tree beside a built one")


def test_every_mesh_worth_the_device_emit_declined(product_lib, monkeypatch):
    """The builder declines the only mesh: no tree of the upload is on the device, the host writes the whole arena - what it writes
    under YCGE_MESH_EMIT_HOST=1, and what ycge_host_mesh_arena_treelets lays out for the same triangles."""
    flat, same40 = _declined_flat(False)
    assert flat.meshes[0].material == 0          # (the hook below emits material 0)
    d, h = _upload(flat, monkeypatch, False, DECLINING), _upload(flat, monkeypatch, True, DECLINING)
    print("device emit:", d[3], d[4], "host emit:", h[3], h[4])
    assert d[4]["host_fallbacks"] == 1 and d[4]["device_builds"] == 0, d[4]
    assert d[3]["device_meshes"] == 0 and d[3]["host_meshes"] == 1 and d[3]["last_device_emit_us"] == 0, d[3]
    _same_arena(d, h, "the only mesh declined")
    hb, hroot, htl = _host(product_lib, same40)
    assert d[1] == htl and np.array_equal(d[0], hb) and d[2][0, 6] == hroot, "the upload's arena against the hook's"


def test_no_treelets_without_the_cooperative_walk(product_lib, monkeypatch):
    flat = _four_mesh_flat()
    arena, tl, meshes, bvh = _same_upload(flat, monkeypatch, (("YCGE_MESH_BVH_DEVICE_MIN", "1"), ("YCGE_NO_COOP", "1")), "YCGE_NO_COOP")
    assert tl == 0 and len(arena) % 32 == 0


@pytest.mark.parametrize("emit_host", [False, True], ids=["device emit", "host emit"])
def test_a_material_out_of_range_is_the_hosts_refusal(product_lib, monkeypatch, emit_host):
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", "1")
    if emit_host: monkeypatch.setenv("YCGE_MESH_EMIT_HOST", "1")
    good, bad = _four_mesh_flat(), _four_mesh_flat(bad_material=True)
    g = RaytraceRenderer(None, 64, 36, 55.0, 1)
    with pytest.raises(abi.YcgeError) as e:
        g.UploadScene(bad)
    assert e.value.status == abi.YCGE_ERR_INVALID_ARG and "mesh 2: triangle material out of range" in str(e.value)
    with pytest.raises(abi.YcgeError) as e:          # no scene afterwards
        g.read_mesh_arena()
    assert e.value.status == abi.YCGE_ERR_NO_SCENE
    with pytest.raises(abi.YcgeError) as e:
        g.TryFlipAndBlit()
    assert e.value.status == abi.YCGE_ERR_NO_SCENE
    g.UploadScene(good)          # and the context takes the next scene
    assert g.mesh_emit_stats()["host_meshes" if emit_host else "device_meshes"] == 4
    g.close()


def _frame_parity(o, g, label):
    o.render(stages=1, threads=16); g.TryFlipAndBlit()
    st = pu.compare_frame(o, g)
    for k in ("rays", "prim_id", "sub_id", "hit_t", "rng_state", "sky", "g_depth", "current_hdr", "taa_history", "g_albedo", "g_normal"):
        assert st[k + "_mismatch"] == 0, f"{label}: {k} differs in {st[k + '_mismatch']} elements"
    for k in ("n_rays", "n_box", "n_tri", "n_prim", "n_vox"):
        assert st[k][0] == st[k][1], f"{label}: counter {k}"


@pytest.fixture(scope="module")
def config_3():
    sc, w, h, ss, pose = scenes.config_scene(3)
    return sc, flatten(sc), pose


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one device", "two devices"])
def test_config_3_rendered_from_a_device_made_arena(product_lib, oracle, monkeypatch, config_3, devices):
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", "1")
    monkeypatch.delenv("YCGE_MESH_EMIT_HOST", raising=False)
    sc, flat, pose = config_3
    o = oracle.OracleRenderer(sc, 96, 54, 1, pose, flat=flat)
    kw = dict(devices=devices) if devices else {}
    g = RaytraceRenderer(flat, 96, 54, pose["fov"], 1, capture_debug=True, count_work=True, **kw)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    st = g.mesh_emit_stats()
    assert st["device_meshes"] == 1 and st["host_meshes"] == 0 and st["arena_bytes"] > 0, st
    for f in (1, 2, 3):
        _frame_parity(o, g, f"config 3, frame {f}")
    if devices:          # the peer's arena is the root's, copied device to device
        fn = g.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int32]
        peer = fn(g.ctx, 0)
        assert peer
        rd = g.L.ycge_debug_read_mesh_arena
        rd.restype, rd.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_read_mesh_arena"]
        mine, tl = g.read_mesh_arena()
        theirs = np.zeros(len(mine), np.uint8); ptl = C.c_uint32(0)
        assert rd(peer, theirs.ctypes.data, len(theirs), C.byref(ptl)) == len(mine) and ptl.value == tl
        assert np.array_equal(mine, theirs)
    o.close(); g.close()


def test_config_3_under_the_host_knob_reports_the_host(product_lib, monkeypatch, config_3):
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", "1")
    monkeypatch.setenv("YCGE_MESH_EMIT_HOST", "1")
    sc, flat, pose = config_3
    g = RaytraceRenderer(flat, 96, 54, pose["fov"], 1)
    st, bvh = g.mesh_emit_stats(), g.mesh_bvh_stats()
    assert st["device_meshes"] == 0 and st["host_meshes"] == 1 and bvh["device_builds"] == 1, (st, bvh)
    g.close()


def _live(L):
    out = (C.c_int64 * 6)()
    assert L.ycge_debug_live_resources(out) == abi.YCGE_OK
    return list(out)


def test_nothing_is_left_behind(product_lib, monkeypatch):
    """create / upload / upload again / destroy on the device path: what the library holds is what it held before."""
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", "1")
    monkeypatch.delenv("YCGE_MESH_EMIT_HOST", raising=False)
    flat = _four_mesh_flat()
    before = _live(product_lib)
    g = RaytraceRenderer(flat, 64, 36, 55.0, 1)
    held = _live(product_lib)
    g.UploadScene(flat)
    assert g.mesh_emit_stats()["device_meshes"] == 4
    assert _live(product_lib)[:2] == held[:2], "the second upload holds what the first held: the emit's buffers are given back"
    g.close()
    assert _live(product_lib) == before


def test_below_the_emit_threshold_the_host_writes_the_arena(product_lib, monkeypatch):
    """YCGE_MESH_EMIT_DEVICE_MIN: trees built on the device, of meshes all smaller than it - the host's emit, as before; one mesh at it - the device's."""
    monkeypatch.setenv("YCGE_MESH_BVH_DEVICE_MIN", "1")
    monkeypatch.delenv("YCGE_MESH_EMIT_HOST", raising=False)
    flat = _four_mesh_flat()
    for emit_min, on_device in (("3001", False), ("3000", True), (None, False)):
        if emit_min is None: monkeypatch.delenv("YCGE_MESH_EMIT_DEVICE_MIN", raising=False)
        else: monkeypatch.setenv("YCGE_MESH_EMIT_DEVICE_MIN", emit_min)
        g = RaytraceRenderer(flat, 64, 36, 55.0, 1)
        st, bvh = g.mesh_emit_stats(), g.mesh_bvh_stats()
        assert bvh["device_builds"] == 3
        assert (st["device_meshes"], st["host_meshes"]) == ((4, 0) if on_device else (0, 4)), (emit_min, st)
        g.close()
