"""OBJ meshes parsed on the device (ycge_obj_parse / _read / _triangles, csrc/ycge_obj.hip) against tests/obj_restatement.py and against
the library's host parser, bit for bit (uint32 views of the floats; bounds as values).  Every file inside the kernels' domain must be
parsed BY the kernels (ycge_debug_obj_stats): a fallback cannot hide a kernel fault."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import obj_cases
import obj_restatement as R
import parity_util as pu
from yetanotherconsolegameengine_amd import abi, mesh_loader
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import AmbientLight, Checker, Material, Mesh, Plane, PointLight, Scene, Sphere, flatten, vec3

pytestmark = pytest.mark.gpu

POSE = dict(pos=(0.3, 1.1, 0.0), yaw=0.05, pitch=-0.15, fov=50.0)


def small_scene(tris=None):
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Objects.append(Plane(vec3(0, 0, 0), vec3(0, 1, 0), Checker(vec3(0.8, 0.8, 0.8), vec3(0.25, 0.25, 0.25), 0.7), 0.0, 0.0))
    if tris is None:
        s.Objects.append(Sphere(vec3(0.0, 0.6, -3.0), 0.6, Material(vec3(0.85, 0.4, 0.2))))
    else:
        s.Objects.append(Mesh(tris, Material(vec3(0.85, 0.4, 0.2))))
    s.Lights.append(PointLight(vec3(2.0, 4.0, 0.0), vec3(1, 1, 1), 60.0))
    return s


def new_renderer(scene=None, w=32, h=18, **kw):
    """a context that hands every file to the kernels (YCGE_OBJ_DEVICE_MIN = 0; the knobs are read once, at ycge_create) unless the test
    has set the knob itself: the test files are far below any measured crossover"""
    mine = "YCGE_OBJ_DEVICE_MIN" not in os.environ
    if mine:
        os.environ["YCGE_OBJ_DEVICE_MIN"] = "0"
    try:
        g = RaytraceRenderer(flatten(scene) if scene is not None else None, w, h, POSE["fov"], 1, **kw)
    finally:
        if mine:
            del os.environ["YCGE_OBJ_DEVICE_MIN"]
    g.SetCamera(POSE["pos"], POSE["yaw"], POSE["pitch"])
    return g


@pytest.fixture(scope="module")
def g(product_lib):
    r = new_renderer(small_scene())
    yield r
    r.close()


@pytest.fixture(scope="module")
def geo(product_lib):
    return abi.obj_geometry(product_lib)


def refusal_of(message: str):
    m = re.search(r"OBJ line (\d+):", message)
    if m:
        return "line", int(m.group(1))
    m = re.search(r"OBJ triangle (\d+) ", message)
    if m:
        return "triangle", int(m.group(1))
    return ("none", None) if "no position or no triangle" in message else ("?", None)


def check_file(g, data, on_device, decline=None, label=""):
    """parse on the context; who parsed; positions, faces, info, default triangles and bounds against the restatement and the host parser"""
    want_pos, want_faces, want_lines = R.parse(data)
    host_pos, host_faces, host_info = abi.obj_parse_host(data, g.L)
    before = g.obj_stats()
    info = g.ParseObj(data)
    after = g.obj_stats()
    if on_device:
        assert info.on_device == 1 and after["device_parses"] == before["device_parses"] + 1 and after["host_parses"] == before["host_parses"] and after["last_decline"] == 0, (label, after)
    else:
        assert info.on_device == 0 and after["host_parses"] == before["host_parses"] + 1 and after["device_parses"] == before["device_parses"], (label, after)
        if decline is not None:
            assert after["last_decline"] == decline, (label, after)
    assert (info.n_positions, info.n_triangles, info.n_lines) == (len(want_pos), len(want_faces), want_lines) == (host_info.n_positions, host_info.n_triangles, host_info.n_lines), label
    pos, faces = g.ReadObj()
    assert np.array_equal(pos.view(np.uint32), want_pos) and np.array_equal(pos.view(np.uint32), host_pos.view(np.uint32)), label
    assert np.array_equal(faces, want_faces) and np.array_equal(faces, host_faces), label
    tris, bounds = g.ObjTriangles()
    want_tris, want_bounds = R.triangles(want_pos, want_faces)
    assert np.array_equal(tris.view(np.uint32), want_tris.view(np.uint32)), label
    assert np.array_equal(bounds, want_bounds), (label, bounds, want_bounds)
    return info


@pytest.mark.parametrize("name", sorted(obj_cases.CASES))
def test_device_parse_equals_restatement_and_host_parser(g, name):
    data, in_domain = obj_cases.CASES[name]
    check_file(g, data, in_domain, None if in_domain else abi.OBJ_DECLINE_FLOAT_DOMAIN, name)


def test_tile_edges(g, geo):
    T = geo["tile_bytes"]
    tri, tri_crlf = obj_cases.TRI, obj_cases.TRI.replace(b"\n", b"\r\n")
    for size in (T - 1, T, T + 1, 3 * T + 5):
        data = obj_cases.padded_to(tri, size)
        assert len(data) == size
        check_file(g, data, True, label=f"{size} bytes")
    check_file(g, obj_cases.at_offset(tri, T - 12), True, label="a line straddles the tile edge")          # "v -4 5 6" starts at T - 4
    check_file(g, obj_cases.at_offset(tri, T - 8), True, label="a line ends on the tile edge")               # its \n is byte T - 1
    check_file(g, obj_cases.at_offset(tri_crlf, T - 8), True, label="\\r closes a tile, \\n opens the next")
    check_file(g, obj_cases.at_offset(tri.replace(b"\n", b"\r"), T - 8), True, label="a lone \\r closes a tile")
    check_file(g, obj_cases.at_offset(tri_crlf, 3 * T - 8)[:-1], True, label="a lone \\r is the file's last byte, third tile")
    check_file(g, b"\xef\xbb\xbf" + obj_cases.at_offset(tri, T - 3), True, label="byte-order mark, a line starts on the tile edge")


def test_line_counts_around_a_wavefront_and_a_workgroup(g, geo):
    Lw = geo["lines_per_workgroup"]
    for k in (2, 63, 64, 65, Lw - 1, Lw, Lw + 1, 2 * Lw + 1):
        info = check_file(g, obj_cases.n_lines_file(k), True, label=f"{k} lines")
        assert info.n_lines == k and info.n_positions == k - 1 and info.n_triangles == 1
    one = obj_cases.n_lines_file(1)          # one line: the kernels run, and the file is refused as the host parser refuses it
    before = g.obj_stats()
    with pytest.raises(abi.YcgeError) as e:
        g.ParseObj(one)
    assert e.value.status == abi.YCGE_ERR_INVALID_ARG and refusal_of(str(e.value)) == ("none", None)
    assert g.obj_stats()["last_decline"] == 0 and g.obj_stats()["host_parses"] == before["host_parses"]


def test_more_tiles_and_more_lines_than_one_scan_trip(g, geo):
    data = obj_cases.many_lines_file()
    assert len(data) > 256 * geo["tile_bytes"] and data.count(b"\n") > 256 * geo["lines_per_workgroup"]
    check_file(g, data, True, label="66 000 lines")


def test_ngon_at_the_line_cap_and_one_byte_over(g, geo):
    cap = geo["line_cap"]
    info = check_file(g, obj_cases.ngon_line(cap), True, label="an n-gon at the cap")
    assert info.n_triangles == (cap - 1) // 2 - 2
    check_file(g, obj_cases.ngon_line(cap + 1), False, abi.OBJ_DECLINE_LINE_CAP, "one byte over the cap")
    check_file(g, b"#" + b"c" * (4 * cap) + b"\n" + obj_cases.TRI, True, label="a comment may be longer than the cap")


@pytest.mark.parametrize("name", sorted(obj_cases.REFUSALS))
def test_refusals_on_the_device_path_are_the_host_parsers(g, name):
    data, status, kind, number = obj_cases.REFUSALS[name]
    with pytest.raises(abi.YcgeError) as host:
        abi.obj_parse_host(data, g.L)
    before = g.obj_stats()
    with pytest.raises(abi.YcgeError) as dev:
        g.ParseObj(data)
    after = g.obj_stats()
    assert after["last_decline"] == 0 and after["host_parses"] == before["host_parses"], after          # the kernels refused it themselves
    assert dev.value.status == status == host.value.status
    assert refusal_of(str(dev.value)) == (kind, number) == refusal_of(str(host.value)), (str(dev.value), str(host.value))
    assert str(dev.value) == str(host.value)
    with pytest.raises(abi.YcgeError) as e:          # nothing is held
        g.ReadObj()
    assert e.value.status == abi.YCGE_ERR_INVALID_ARG
    check_file(g, obj_cases.TRI, True, label="a good file after the refusal")          # the context stays usable: it parses ...
    g.TryFlipAndBlit()                                                                   # ... and renders


def test_argument_refusals(g):
    info = abi.ObjInfo()
    assert g.L.ycge_obj_parse(g.ctx, None, 10, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert g.L.ycge_obj_parse(g.ctx, b"", 0, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert g.L.ycge_obj_parse(g.ctx, b"v", 1 << 31, C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert g.L.ycge_obj_parse(g.ctx, obj_cases.TRI, len(obj_cases.TRI), None) == abi.YCGE_ERR_INVALID_ARG
    assert g.L.ycge_obj_parse(None, obj_cases.TRI, len(obj_cases.TRI), C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    g.ParseObj(obj_cases.TRI)
    assert g.L.ycge_obj_triangles(g.ctx, 1, 1.0, 1.0, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    tris = np.zeros((1, 3, 3), np.float32)
    assert g.L.ycge_obj_triangles(g.ctx, 0, 1.0, 1.0, None, tris.ctypes.data, None) == abi.YCGE_OK          # translate NULL = 0, no bounds asked
    assert tris.reshape(-1).tolist() == [1, 2, 3, -4, 5, 6, 7, -8, 9]
    assert g.L.ycge_obj_read(g.ctx, None, None) == abi.YCGE_OK


def test_tail_three_times_on_one_held_obj_and_auto_ground(g):
    data = obj_cases.CASES["drawn_mixed_2"][0]
    want_pos, want_faces, _ = R.parse(data)
    g.ParseObj(data)
    for kw in (dict(normalize=True, target_size=1.0, scale=1.0, translate=(0.0, 0.0, 0.0)),            # the transform is skipped
               dict(normalize=False, target_size=1.0, scale=1.0, translate=(0.0, 0.0, 0.0)),           # nothing but the gather
               dict(normalize=True, target_size=2.5, scale=0.75, translate=(1.5, -2.0, 0.25)),
               dict(normalize=False, target_size=1.0, scale=1.0, translate=(0.0, 0.5, 0.0))):          # scale == 1, t != 0: the transform runs
        tris, bounds = g.ObjTriangles(**kw)
        want, want_bounds = R.triangles(want_pos, want_faces, **kw)
        assert np.array_equal(tris.view(np.uint32), want.view(np.uint32)), kw
        assert np.array_equal(bounds, want_bounds), kw
    # MeshScenes.AddMeshAutoGround with one parse, on the hull
    pos, faces, _ = abi.obj_parse_host(obj_cases.HULL, g.L)
    want = mesh_loader.add_mesh_auto_ground(pos, faces, 1.4, (0.0, 0.0, -3.0))
    before = g.obj_stats()["device_parses"]
    got = mesh_loader.add_mesh_auto_ground_device(g, obj_cases.HULL, 1.4, (0.0, 0.0, -3.0))
    assert g.obj_stats()["device_parses"] == before + 1
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    got = mesh_loader.from_obj_device(g, obj_cases.HULL, scale=2.0, translate=(1, 0, 0))
    assert np.array_equal(got.view(np.uint32), mesh_loader.from_obj_arrays(pos, faces, scale=2.0, translate=(1, 0, 0)).view(np.uint32))


def test_a_path_is_read_and_page_locked_text_goes_up_directly(g, tmp_path):
    path = tmp_path / "hull.obj"
    path.write_bytes(obj_cases.HULL)
    info = g.ParseObj(path)
    assert info.on_device == 1 and info.n_positions == 6 and info.n_triangles == 11
    want = g.ReadObj()
    p = C.c_void_p()
    n = len(obj_cases.HULL)
    assert g.L.ycge_alloc_host_buffer(n, C.byref(p)) == abi.YCGE_OK
    try:
        C.memmove(p, obj_cases.HULL, n)
        info = abi.ObjInfo()
        g._check(g.L.ycge_obj_parse(g.ctx, p, n, C.byref(info)))
        g._obj_info = info
        got = g.ReadObj()
        assert info.on_device == 1 and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    finally:
        g.ReleaseObj()
        assert g.L.ycge_free_host_buffer(p) == abi.YCGE_OK


BUFFERS = (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY)


def test_a_parse_between_frames_changes_no_frame(product_lib):
    def three_frames(parse):
        r = new_renderer(small_scene())
        r.TryFlipAndBlit(); r.TryFlipAndBlit()
        if parse:
            r.ParseObj(obj_cases.CASES["drawn_mixed_0"][0])
            r.ObjTriangles(scale=2.0)
        sdr = r.TryFlipAndBlit(want_sdr=True).copy()
        out = [r.read(b).copy() for b in BUFFERS] + [sdr, np.int64(r.stats.frame)]
        r.close()
        return out
    for a, b in zip(three_frames(True), three_frames(False)):
        assert pu.bits_equal(a, b)


def test_parsed_triangles_render_as_mesh_loaders_do(product_lib, oracle):
    pos, faces, _ = abi.obj_parse_host(obj_cases.HULL, product_lib)
    want = mesh_loader.add_mesh_auto_ground(pos, faces, 1.4, (0.0, 0.0, -3.0))
    r = new_renderer(None)
    tris = mesh_loader.add_mesh_auto_ground_device(r, obj_cases.HULL, 1.4, (0.0, 0.0, -3.0))
    r.close()
    assert np.array_equal(tris.view(np.uint32), want.view(np.uint32))
    o, g2 = pu.run_pair(oracle, small_scene(tris), 64, 36, 1, POSE, frames=1)
    st = pu.compare_frame(o, g2)
    for k in ("rays", "prim_id", "sub_id", "hit_t", "rng_state", "sky", "g_depth", "current_hdr", "taa_history", "g_albedo", "g_normal"):
        assert st[k + "_mismatch"] == 0, (k, st[k + "_mismatch"])
    assert (g2.read(abi.BUF_PRIM_ID) == 1).any()          # the mesh is in view
    o2, g3 = pu.run_pair(oracle, small_scene(want), 64, 36, 1, POSE, frames=1)
    for b in BUFFERS:
        assert pu.bits_equal(g2.read(b), g3.read(b))
    for x in (o, g2, o2, g3):
        x.close()


def _live(L):
    out = (C.c_int64 * 6)()
    assert L.ycge_debug_live_resources(out) == abi.YCGE_OK
    return list(out)


def test_lifecycle(product_lib):
    base = _live(product_lib)
    r = new_renderer(None)
    a = r.ParseObj(obj_cases.HULL)
    b = r.ParseObj(obj_cases.TRI)          # replaces
    assert (a.n_positions, a.n_triangles) == (6, 11) and (b.n_positions, b.n_triangles) == (3, 1)
    pos, faces = r.ReadObj()
    assert pos.shape == (3, 3) and faces.tolist() == [[0, 1, 2]]
    r.ReleaseObj()
    for call in (r.ReadObj, r.ObjTriangles):          # refused after the release
        with pytest.raises(abi.YcgeError) as e:
            call()
        assert e.value.status == abi.YCGE_ERR_INVALID_ARG and "holds no parsed OBJ" in str(e.value)
    r.ReleaseObj()          # releasing nothing is fine
    r.ParseObj(obj_cases.CASES["drawn_mixed_2"][0])
    r.ObjTriangles()
    assert _live(product_lib)[1] > base[1]
    r.close()          # destroyed with an OBJ held: everything goes with the context
    assert _live(product_lib) == base


def test_host_knob_and_device_min(product_lib, monkeypatch):
    data = obj_cases.CASES["drawn_mixed_0"][0]
    monkeypatch.setenv("YCGE_OBJ_HOST", "1")
    r = new_renderer(None)          # (the knobs are read once, at ycge_create)
    check_file(r, data, False, abi.OBJ_DECLINE_ENV_HOST, "YCGE_OBJ_HOST")
    r.close()
    monkeypatch.delenv("YCGE_OBJ_HOST")
    # the default: the crossover written into csrc/ycge_ctx.h
    default = abi.obj_geometry(product_lib)["device_min"]
    r = RaytraceRenderer(None, 32, 18)
    if default > len(obj_cases.TRI):
        check_file(r, obj_cases.TRI, False, abi.OBJ_DECLINE_BELOW_MIN, "below the default YCGE_OBJ_DEVICE_MIN")
    if default < 1 << 21:
        check_file(r, obj_cases.padded_to(obj_cases.TRI, max(default, 64)), True, label="at the default YCGE_OBJ_DEVICE_MIN")
    r.close()
    monkeypatch.setenv("YCGE_OBJ_HOST", "1")
    monkeypatch.delenv("YCGE_OBJ_HOST")
    monkeypatch.setenv("YCGE_OBJ_DEVICE_MIN", str(len(data) + 1))
    r = new_renderer(None)
    check_file(r, data, False, abi.OBJ_DECLINE_BELOW_MIN, "below YCGE_OBJ_DEVICE_MIN")
    check_file(r, data + b"\n", True, label="at YCGE_OBJ_DEVICE_MIN")
    r.close()


def test_a_peer_context_refuses_and_the_root_parses(product_lib):
    r = new_renderer(None, devices=[0, 0])
    fn = r.L.ycge_debug_peer_context
    fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int32]
    peer = fn(r.ctx, 0)
    assert peer
    info = abi.ObjInfo()
    assert r.L.ycge_obj_parse(peer, obj_cases.TRI, len(obj_cases.TRI), C.byref(info)) == abi.YCGE_ERR_INVALID_ARG
    assert b"peer contexts" in r.L.ycge_last_error(peer)
    assert r.L.ycge_obj_release(peer) == abi.YCGE_ERR_INVALID_ARG and r.L.ycge_obj_read(peer, None, None) == abi.YCGE_ERR_INVALID_ARG
    check_file(r, obj_cases.HULL, True, label="the root of a two-device context")
    r.close()
