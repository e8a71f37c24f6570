"""MeshScenes.AddMeshAutoGround on the device (ycge_obj_ground / ycge_obj_triangles_auto_ground, csrc/ycge_obj_ground.hip) against
tests/obj_ground_restatement.py and against the library's host tail, bit for bit (uint32 views of the floats, every integer field).
Every OBJ must be labelled and summed BY the kernels (on_device == 1 and ycge_debug_obj_ground_stats): a fallback cannot hide a kernel
fault."""
import ctypes as C
import os

import numpy as np
import pytest

import obj_ground_cases as cases
import obj_ground_restatement as R
import obj_restatement
import parity_util as pu
from obj_ground_cases import want_of
from obj_ground_restatement import want_words, words
from yetanotherconsolegameengine_amd import abi, mesh_loader
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import AmbientLight, Checker, Material, Plane, PointLight, Scene, Sphere, flatten, vec3

pytestmark = pytest.mark.gpu

POSE = dict(pos=(0.3, 1.1, 0.0), yaw=0.05, pitch=-0.15, fov=50.0)
PLACE = (1.4, (0.25, -0.5, -3.0))          # scale, targetPos


def small_scene():
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Objects.append(Plane(vec3(0, 0, 0), vec3(0, 1, 0), Checker(vec3(0.8, 0.8, 0.8), vec3(0.25, 0.25, 0.25), 0.7), 0.0, 0.0))
    s.Objects.append(Sphere(vec3(0.0, 0.6, -3.0), 0.6, Material(vec3(0.85, 0.4, 0.2))))
    s.Lights.append(PointLight(vec3(2.0, 4.0, 0.0), vec3(1, 1, 1), 60.0))
    return s


def new_renderer(scene=None, w=32, h=18, **kw):
    """a context that hands every file and every held OBJ to the kernels (YCGE_OBJ_DEVICE_MIN = YCGE_OBJ_GROUND_DEVICE_MIN = 0; the knobs are
    read once, at ycge_create) unless the test has set a knob itself: the test meshes are far below any measured crossover"""
    mine = [k for k in ("YCGE_OBJ_DEVICE_MIN", "YCGE_OBJ_GROUND_DEVICE_MIN") if k not in os.environ]
    for k in mine:
        os.environ[k] = "0"
    try:
        g = RaytraceRenderer(flatten(scene) if scene is not None else None, w, h, POSE["fov"], 1, **kw)
    finally:
        for k in mine:
            del os.environ[k]
    g.SetCamera(POSE["pos"], POSE["yaw"], POSE["pitch"])
    return g


@pytest.fixture(scope="module")
def g(product_lib):
    r = new_renderer(small_scene())
    yield r
    r.close()


@pytest.fixture(scope="module")
def g2(product_lib):
    r = new_renderer(None)
    yield r
    r.close()


def placed(pos, faces, min_y):
    """AddMeshAutoGround's triangles by tests/obj_restatement.py, from a normalised min.y"""
    scale, target = PLACE
    t = (np.float32(target[0]), R.y_translate(min_y, scale, target[1]), np.float32(target[2]))
    return obj_restatement.triangles(np.ascontiguousarray(pos, np.float32).view(np.uint32), faces, normalize=True, target_size=1.0, scale=scale, translate=t)


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_tail_equals_the_restatement_and_the_host_tail(g, g2, name):
    c, want = cases.get(name), want_words(want_of(name))
    info = g.ParseObj(c.text)
    assert info.on_device == (1 if c.device_parse else 0), name          # (the one host-PARSED case still runs the device tail: the held arrays are on the device whoever parsed)
    pos, faces = g.ReadObj()
    assert np.array_equal(pos.view(np.uint32), c.pos.view(np.uint32)) and np.array_equal(faces, c.faces)
    host = abi.obj_ground_host(pos, faces, g.L)
    before = g.obj_ground_stats()
    got = g.ObjGround()
    after = g.obj_ground_stats()
    print(name, "device", words(got), "host", words(host), after)
    assert got.on_device == 1 and got.reserved == 0, (name, after)
    assert after["device_tails"] == before["device_tails"] + 1 and after["host_tails"] == before["host_tails"] and after["last_decline"] == 0, (name, after)
    assert 1 <= after["rounds"] < 64 and after["serial_sums"] == 0, (name, after)          # neighbour-to-neighbour propagation would need about 2^15 rounds on the strips
    assert words(got) == want, (name, words(got), want)
    assert words(got) == words(host), name
    again = g.ObjGround()          # the same answer each time ...
    assert words(again) == want and again.on_device == 1
    g2.ParseObj(c.text)            # ... and on a second context
    other = g2.ObjGround()
    assert words(other) == want and other.on_device == 1
    # the one call: AddMeshAutoGround's triangles
    scale, target = PLACE
    tris, bounds, ground = g.ObjTrianglesAutoGround(scale, target)
    assert words(ground) == want and ground.on_device == 1, name
    want_tris, want_bounds = placed(c.pos, c.faces, want_of(name)["min"][1])
    assert np.array_equal(tris.view(np.uint32), want_tris.view(np.uint32)), name
    assert np.array_equal(bounds, want_bounds, equal_nan=True), (name, bounds, want_bounds)
    assert g.obj_ground_stats()["device_tails"] == after["device_tails"] + 2


@pytest.mark.parametrize("name", [n for n in cases.SMALL if n not in cases.NAN_CENTROID])
def test_the_one_call_equals_mesh_loader_on_the_host_parsers_arrays(g, name):
    """(mesh_loader takes its extremes with np.min / np.max, which hand a NaN on where the reference's compares do not: cases.NAN_CENTROID is
    held to the restatements above)"""
    c = cases.get(name)
    scale, target = PLACE
    pos, faces, _ = abi.obj_parse_host(c.text, g.L)
    want = mesh_loader.add_mesh_auto_ground(pos, faces, scale, target)
    before = g.obj_stats()["device_parses"]
    got = mesh_loader.add_mesh_auto_ground_device(g, c.text, scale, target)
    assert g.obj_stats()["device_parses"] == before + 1          # one parse, on the device
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert g.obj_ground_stats()["last_decline"] == 0


def test_host_knob_and_device_min_give_the_same_bits(product_lib, monkeypatch):
    name = "winner_257"
    c, want = cases.get(name), want_words(want_of(name))
    n = len(c.faces)

    def run(decline, on_device):
        r = new_renderer(None)          # (the knobs are read once, at ycge_create)
        try:
            r.ParseObj(c.text)
            got = r.ObjGround()
            st = r.obj_ground_stats()
            assert got.on_device == on_device and words(got) == want, (decline, st)
            assert st["last_decline"] == decline and (st["device_tails"], st["host_tails"]) == ((1, 0) if on_device else (0, 1)), st
            tris, _, ground = r.ObjTrianglesAutoGround(*PLACE)
            assert ground.on_device == on_device and words(ground) == want
            assert np.array_equal(tris.view(np.uint32), placed(c.pos, c.faces, want_of(name)["min"][1])[0].view(np.uint32))
        finally:
            r.close()

    monkeypatch.setenv("YCGE_OBJ_GROUND_HOST", "1")
    run(abi.OBJ_GROUND_DECLINE_ENV_HOST, 0)
    monkeypatch.delenv("YCGE_OBJ_GROUND_HOST")
    monkeypatch.setenv("YCGE_OBJ_GROUND_DEVICE_MIN", str(n + 1))
    run(abi.OBJ_GROUND_DECLINE_BELOW_MIN, 0)
    monkeypatch.setenv("YCGE_OBJ_GROUND_DEVICE_MIN", str(n))
    run(0, 1)
    monkeypatch.delenv("YCGE_OBJ_GROUND_DEVICE_MIN")
    # the default written into csrc/ycge_ctx.h decides for a context made with nothing set
    default = abi.obj_ground_geometry(product_lib)["device_min_default"]
    r = RaytraceRenderer(None, 32, 18)
    try:
        r.ParseObj(c.text)
        got = r.ObjGround()
        assert words(got) == want and got.on_device == (1 if n >= default else 0)
    finally:
        r.close()


def test_refusals_peer_context_and_no_held_obj(product_lib):
    r = new_renderer(None, devices=[0, 0])
    try:
        fn = r.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int32]
        peer = fn(r.ctx, 0)
        assert peer
        info = abi.ObjGroundInfo()
        tris = np.zeros((1, 3, 3), np.float32)
        target = (C.c_float * 3)(0, 0, 0)
        with pytest.raises(abi.YcgeError) as e:          # nothing is held yet
            r.ObjGround()
        assert e.value.status == abi.YCGE_ERR_INVALID_ARG and "holds no parsed OBJ" in str(e.value)
        assert r.L.ycge_obj_triangles_auto_ground(r.ctx, 1.0, target, tris.ctypes.data, None, None) == abi.YCGE_ERR_INVALID_ARG
        assert b"holds no parsed OBJ" in r.L.ycge_last_error(r.ctx)
        c = cases.get("one_triangle")
        r.ParseObj(c.text)
        assert r.L.ycge_obj_ground(peer, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG and b"peer contexts" in r.L.ycge_last_error(peer)
        assert r.L.ycge_obj_triangles_auto_ground(peer, 1.0, target, tris.ctypes.data, None, None) == abi.YCGE_ERR_INVALID_ARG
        assert r.L.ycge_obj_ground(r.ctx, None) == abi.YCGE_ERR_INVALID_ARG
        assert r.L.ycge_obj_triangles_auto_ground(r.ctx, 1.0, None, tris.ctypes.data, None, None) == abi.YCGE_ERR_INVALID_ARG
        assert r.L.ycge_obj_triangles_auto_ground(r.ctx, 1.0, target, None, None, None) == abi.YCGE_ERR_INVALID_ARG
        assert r.L.ycge_obj_triangles_auto_ground(r.ctx, 1.0, target, tris.ctypes.data, None, None) == abi.YCGE_OK          # no bounds, no info asked
        got = r.ObjGround()          # the root of a two-device context runs the tail
        assert got.on_device == 1 and words(got) == want_words(want_of("one_triangle"))
        r.ReleaseObj()
        with pytest.raises(abi.YcgeError) as e:
            r.ObjTrianglesAutoGround(*PLACE)
        assert e.value.status == abi.YCGE_ERR_INVALID_ARG and "holds no parsed OBJ" in str(e.value)
    finally:
        r.close()


BUFFERS = (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY)


def test_a_tail_between_frames_changes_no_frame(product_lib):
    def three_frames(tail):
        r = new_renderer(small_scene())
        r.TryFlipAndBlit(); r.TryFlipAndBlit()
        if tail:
            r.ParseObj(cases.get("winner_1025").text)
            assert r.ObjGround().on_device == 1
            r.ObjTrianglesAutoGround(*PLACE)
        sdr = r.TryFlipAndBlit(want_sdr=True).copy()
        out = [r.read(b).copy() for b in BUFFERS] + [sdr, np.int64(r.stats.frame)]
        r.close()
        return out
    for a, b in zip(three_frames(True), three_frames(False)):
        assert pu.bits_equal(a, b)


def _live(L):
    out = (C.c_int64 * 6)()
    assert L.ycge_debug_live_resources(out) == abi.YCGE_OK
    return list(out)


def test_lifecycle(product_lib):
    base = _live(product_lib)
    r = new_renderer(None)
    r.ParseObj(cases.get("winner_257").text)
    parsed = _live(product_lib)
    assert r.ObjGround().on_device == 1
    held = _live(product_lib)
    assert held[0] > parsed[0] and held[1] > parsed[1]          # the tail's buffers belong to the held OBJ ...
    r.ParseObj(cases.get("one_triangle").text)                   # ... and leave with it
    assert _live(product_lib)[0] < held[0]
    assert r.ObjGround().component_faces == 1
    r.ReleaseObj()
    assert _live(product_lib)[0] <= parsed[0]
    r.ParseObj(cases.get("winner_63").text)
    r.ObjTrianglesAutoGround(*PLACE)
    r.close()          # destroyed with an OBJ and its tail buffers held: everything goes with the context
    assert _live(product_lib) == base
