"""-m gpu: the HIP path against the oracle through the C-ABI, on the same seeded inputs.

Bars (north_star / SURVEY 8d): primary hit index and t bit-exact, integer RNG state bit-exact,
traversal counters equal, radiance RMS <= 1e-4 — the implementation is in fact bit-exact on every
buffer, which the tests report and the strict ones require.  Every test runs on both device paths
(wavefront stage pipeline and single-launch kernel; YCGE_PATH selects).
"""
import ctypes as C

import numpy as np
import pytest

import parity_util as pu
from pathlib import Path as _Path
GOLDEN_DIR = _Path(__file__).resolve().parent / "golden"          # committed golden buffers (tests/golden/make_fixtures.py)
from yetanotherconsolegameengine_amd import abi, scenes, tiles
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import (AmbientLight, Box, Checker, CylinderY, Disk, Material, Mesh, Plane, PointLight,
                                                   Scene, Solid, Sphere, Texture, Triangle, XYRect, XZRect, YZRect, flatten, vec3, ZERO)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["wavefront", "megakernel"])
def path(request, monkeypatch):
    monkeypatch.setenv("YCGE_PATH", request.param)
    return request.param


def _assert_parity(stats, label, exact=True):
    print(label, stats)
    for k in ("rays", "prim_id", "sub_id", "hit_t", "rng_state", "sky", "g_depth"):
        assert stats[k + "_mismatch"] == 0, f"{label}: {k} differs in {stats[k + '_mismatch']} elements"
    for k in ("current_hdr", "taa_history", "g_albedo", "g_normal"):
        assert stats[k + "_rms"] <= pu.RMS_TOL, f"{label}: {k} RMS {stats[k + '_rms']}"      # north_star tolerance: 1e-4 RMS
        if exact:
            assert stats[k + "_mismatch"] == 0, f"{label}: {k} not bit-exact ({stats[k + '_mismatch']} elements)"
    for k in ("n_rays", "n_box", "n_tri", "n_prim", "n_vox"):
        assert stats[k][0] == stats[k][1], f"{label}: counter {k} oracle {stats[k][0]} != hip {stats[k][1]}"


@pytest.mark.parametrize("cfg_n", [1, 2])
def test_analytic_scenes_three_frames(product_lib, oracle, path, cfg_n):
    sc, w, h, ss, pose = scenes.config_scene(cfg_n)
    o, g = pu.run_pair(oracle, sc, w, h, ss, pose, frames=1)
    _assert_parity(pu.compare_frame(o, g), f"cfg{cfg_n} frame1")
    for f in (2, 3):
        o.render(stages=1, threads=8); g.TryFlipAndBlit()
        _assert_parity(pu.compare_frame(o, g), f"cfg{cfg_n} frame{f}")
    o.close(); g.close()


def test_committed_goldens_on_gpu(product_lib, path):
    """The HIP path against the committed oracle fixture (no oracle run involved)."""
    z = np.load(GOLDEN_DIR / "cornell_80x45_frames123.npz")
    sc, w, h, ss, pose = scenes.config_scene(1)
    with RaytraceRenderer(sc, w, h, pose["fov"], ss, capture_debug=True) as g:
        g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        for frame in (1, 2, 3):
            g.TryFlipAndBlit()
            if frame == 1:
                for name, which in (("rays", abi.BUF_RAYS), ("prim_id", abi.BUF_PRIM_ID), ("sub_id", abi.BUF_SUB_ID), ("hit_t", abi.BUF_HIT_T),
                                    ("current_hdr", abi.BUF_CURRENT_HDR), ("rng_state", abi.BUF_RNG_STATE)):
                    assert pu.bits_equal(g.read(which), z[f"f1_{name}"]), name
            assert pu.bits_equal(g.read(abi.BUF_TAA_HISTORY), z[f"f{frame}_taa_history"]), frame


def test_committed_post_goldens_on_gpu(product_lib, path):
    """The HIP post stage against the committed fixture (no oracle run involved)."""
    z = np.load(GOLDEN_DIR / "cornell_80x45_post.npz")
    sc, w, h, ss, pose = scenes.config_scene(1)
    with RaytraceRenderer(sc, w, h, pose["fov"], ss) as g:
        g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        for frame in (1, 2, 3):
            sdr = g.TryFlipAndBlit(want_sdr=True)
            assert pu.bits_equal(sdr, z[f"f{frame}_sdr"]), frame
            assert np.float32(g.stats.exposure).view(np.uint32) == np.float32(z[f"f{frame}_exposure"]).view(np.uint32)
        assert pu.bits_equal(g.read(abi.BUF_DENOISED), z["f3_denoised"])


def _zoo_scene(transparent: bool):
    """Every primitive class + checker + emissive + a true mirror (>= 0.9) and, optionally, glass."""
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.05)
    s.Add(Plane(vec3(0, 0, 0), vec3(0, 1, 0), Checker(vec3(0.75, 0.75, 0.75), vec3(0.2, 0.2, 0.2), 0.8), 0.05, 0.0))
    s.Add(CylinderY(vec3(-1.2, 0.0, -3.0), 0.6, 0.0, 1.6, True, Material(vec3(0.2, 0.35, 0.9), 0.1, 0.0, ZERO)))
    s.Add(Disk(vec3(1.6, 0.01, -2.2), vec3(0, 1, 0), 0.9, Solid(vec3(0.8, 0.8, 0.1)), 0.0, 0.0))
    s.Add(Triangle(vec3(0.2, 0.0, -3.6), vec3(1.3, 1.4, -3.0), vec3(-0.7, 0.7, -2.8), Material(vec3(0.9, 0.25, 0.25), 0.1, 0.0, ZERO)))
    s.Add(Sphere(vec3(2.4, 0.8, -4.0), 0.8, Material(vec3(0.98, 0.98, 0.98), 0.0, 0.95, ZERO)))             # mirror branch
    s.Add(Box(vec3(-2.8, 0.0, -5.5), vec3(-1.6, 1.2, -4.3), Solid(vec3(0.86, 0.86, 0.86)), 0.1, 0.92))       # mirror via ctor override
    s.Add(XZRect(-0.5, 0.5, -2.6, -2.0, 1.9, Material(vec3(0, 0, 0), 0.0, 0.0, vec3(2.0, 1.8, 1.5)), 0.0, 0.0))  # emissive panel
    if transparent:
        s.Add(Sphere(vec3(0.3, 0.6, -1.9), 0.6, Material(vec3(1, 1, 1), 0.0, 0.05, ZERO, 0.9, 1.5, vec3(0.9, 1.0, 0.9))))
        s.Add(Sphere(vec3(-0.6, 0.4, -1.6), 0.4, Material(vec3(1, 1, 1), 0.0, 0.0, ZERO, 0.6, 1.33, vec3(1.0, 0.8, 0.8))))
    pos, faces = scenes.make_torus_knot(60, 16)
    s.Add(Mesh((pos[faces] * np.float32(0.25) + np.float32([-0.2, 1.9, -3.2])).astype(np.float32), Material(vec3(0.3, 0.8, 0.4))))
    s.Lights.append(PointLight(vec3(-2.2, 3.2, -2.0), vec3(1.0, 0.95, 0.9), 70.0))
    s.Lights.append(PointLight(vec3(2.4, 2.2, -1.4), vec3(0.9, 0.95, 1.0), 60.0))
    s.Lights.append(PointLight(vec3(0.0, 0.5, 3.0), vec3(1, 1, 1), 0.0))       # zero intensity still costs a shadow ray (quirk 8)
    s.BackgroundTop, s.BackgroundBottom = vec3(0.58, 0.78, 1.0), vec3(0.95, 0.98, 1.0)
    return s


def _textured_scene(glass: bool):
    """SURVEY row a9, the texture branch of SampleAlbedo: every Hittable that sets (U, V) - the three rectangles, a box, a Triangle,
    a mesh - and two that leave it (0, 0), with textures of several sizes, weights and UV scales; optionally a glass sphere (its
    reflected path carries the sampled albedo) in front."""
    rng = np.random.default_rng(42)
    big = Texture(rng.integers(0, 256, (32, 48, 4), dtype=np.uint8))
    small = Texture(np.array([[[255, 40, 40], [40, 255, 40], [40, 40, 255]], [[250, 250, 60], [60, 250, 250], [250, 60, 250]]], np.uint8))
    one = Texture(np.array([[[200, 120, 30]]], np.uint8))
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.08)
    s.Add(XZRect(-6.0, 6.0, -12.0, 2.0, 0.0, Material(vec3(0.8, 0.8, 0.8), DiffuseTexture=big, UVScale=3.0), 0.05, 0.0))
    s.Add(XYRect(-5.0, 5.0, 0.0, 4.0, -9.0, Material(vec3(0.3, 0.3, 0.9), DiffuseTexture=small, TextureWeight=0.6, UVScale=2.5), 0.0, 0.0))
    s.Add(YZRect(0.0, 4.0, -9.0, -1.0, -5.0, Material(vec3(0.9, 0.9, 0.9), DiffuseTexture=big, UVScale=0.35), 0.0, 0.0))
    s.Add(Box(vec3(1.5, 0.0, -5.0), vec3(3.0, 1.5, -3.5), Material(vec3(1, 1, 1), DiffuseTexture=small, UVScale=1.0), 0.1, 0.0))
    s.Add(Triangle(vec3(-4.0, 0.2, -6.0), vec3(-1.5, 0.2, -5.0), vec3(-3.0, 2.8, -6.5), Material(vec3(0.5, 0.5, 0.5), DiffuseTexture=big, TextureWeight=0.85, UVScale=4.0)))
    pos, faces = scenes.make_torus_knot(48, 12)
    s.Add(Mesh((pos[faces] * np.float32(0.3) + np.float32([0.0, 1.6, -4.2])).astype(np.float32), Material(vec3(0.9, 0.6, 0.3), DiffuseTexture=big, UVScale=1.0)))
    s.Add(Sphere(vec3(-2.2, 0.7, -3.0), 0.7, Material(vec3(0.2, 0.9, 0.2), DiffuseTexture=one, TextureWeight=0.5)))          # (U, V) = (0, 0)
    s.Add(CylinderY(vec3(3.8, 0.0, -7.0), 0.5, 0.0, 1.8, True, Material(vec3(0.7, 0.7, 0.7), DiffuseTexture=small, TextureWeight=0.0)))   # weight 0: albedo
    if glass:
        s.Add(Sphere(vec3(0.4, 0.6, -2.0), 0.6, Material(vec3(1, 1, 1), 0.0, 0.05, ZERO, 0.9, 1.5, vec3(0.9, 1.0, 0.9), DiffuseTexture=small, UVScale=1.0)))
    s.Lights.append(PointLight(vec3(-2.0, 5.0, -1.0), vec3(1.0, 0.95, 0.9), 90.0))
    s.Lights.append(PointLight(vec3(3.0, 3.0, -2.0), vec3(0.9, 0.95, 1.0), 50.0))
    s.BackgroundTop, s.BackgroundBottom = vec3(0.5, 0.7, 1.0), vec3(0.9, 0.95, 1.0)
    return s


@pytest.mark.parametrize("glass", [False, True])
def test_textured_materials_bit_exact(product_lib, oracle, path, glass):
    """Textured albedo through the G-buffer, the direct light, the bounce and (glass) the reflected path item, three frames; the
    G-buffer albedo must actually vary over the textured floor."""
    pose = dict(pos=(0.2, 1.7, 2.2), yaw=0.04, pitch=-0.22, fov=55.0)
    o, g = pu.run_pair(oracle, _textured_scene(glass), 256, 72, 1, pose, frames=1)
    _assert_parity(pu.compare_frame(o, g), f"textured glass={glass} frame 1")
    for f in (2, 3):
        o.render(stages=1, threads=8); g.TryFlipAndBlit()
        _assert_parity(pu.compare_frame(o, g), f"textured glass={glass} frame {f}")
    alb, pid = g.read(abi.BUF_G_ALBEDO).reshape(-1, 3), g.read(abi.BUF_PRIM_ID).reshape(-1)
    floor = alb[pid == 0]
    assert len(floor) > 500 and len(np.unique(floor.round(3), axis=0)) > 100, "the floor's albedo is not textured"
    assert set(np.unique(pid)) >= {0, 1, 3, 4, 5, 6}
    o.close(); g.close()


def test_live_textures_follow_their_frames(product_lib, oracle, path):
    """LIVE textures (Texture(IFrameReader, ...), Renderer/Texture.cs:51-66): SampleBilinear's other branch (:113-140 - flips, clamped
    neighbours, B, G, R bytes), a new frame before every rendered frame (ycge_scene_update_texture = what GetCurrentFramePtr() shows),
    and Scene.HasDynamicTextures restarting the TAA history each time (RaytraceRenderer.cs:171).  BGR and BGRA, with and without flips,
    on a rectangle, a box and a mesh, beside a static texture; every buffer equals the oracle's, frame after frame."""
    from yetanotherconsolegameengine_amd.scene import LiveTexture
    rng = np.random.default_rng(77)
    cam = LiveTexture(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8))
    video = LiveTexture(rng.integers(0, 256, (9, 16, 4), dtype=np.uint8), flipU=True, flipV=True)
    still = Texture(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8))
    s = Scene()
    s.HasDynamicTextures = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Add(XZRect(-6.0, 6.0, -12.0, 2.0, 0.0, Material(vec3(0.8, 0.8, 0.8), DiffuseTexture=cam, UVScale=2.0), 0.05, 0.0))
    s.Add(Box(vec3(1.5, 0.0, -5.0), vec3(3.0, 1.5, -3.5), Material(vec3(1, 1, 1), DiffuseTexture=video, TextureWeight=0.8), 0.1, 0.0))
    s.Add(XYRect(-5.0, 5.0, 0.0, 4.0, -9.0, Material(vec3(0.3, 0.3, 0.9), DiffuseTexture=still, UVScale=2.5), 0.0, 0.0))
    pos, faces = scenes.make_torus_knot(48, 12)
    s.Add(Mesh((pos[faces] * np.float32(0.3) + np.float32([-1.0, 1.6, -4.2])).astype(np.float32), Material(vec3(0.9, 0.6, 0.3), DiffuseTexture=video, UVScale=3.0)))
    s.Lights.append(PointLight(vec3(-2.0, 5.0, -1.0), vec3(1.0, 0.95, 0.9), 90.0))
    s.BackgroundTop, s.BackgroundBottom = vec3(0.5, 0.7, 1.0), vec3(0.9, 0.95, 1.0)
    pose = dict(pos=(0.2, 1.7, 2.2), yaw=0.04, pitch=-0.22, fov=55.0)
    o, g = pu.run_pair(oracle, s, 256, 72, 1, pose, frames=1)
    _assert_parity(pu.compare_frame(o, g), "live textures, frame 1")
    first = g.read(abi.BUF_G_ALBEDO).copy()
    for f in (2, 3, 4):
        for t in (cam, video):
            t.set_frame(rng.integers(0, 256, t.frame.shape, dtype=np.uint8))
            o.update_texture(t); g.UpdateTexture(t)
        o.render(stages=1, threads=8); g.TryFlipAndBlit()
        _assert_parity(pu.compare_frame(o, g), f"live textures, frame {f}")
        assert g.stats.history_reset == 1
    assert not pu.bits_equal(first, g.read(abi.BUF_G_ALBEDO)), "the new frames did not reach the albedo"
    with pytest.raises(abi.YcgeError):
        g.L.ycge_scene_update_texture.restype = C.c_int
        g._check(g.L.ycge_scene_update_texture(g.ctx, 2, cam.frame.ctypes.data_as(C.c_void_p), cam.frame.nbytes))      # texture 2 is the static one
    o.close(); g.close()


def test_a_single_textured_mesh_takes_the_generic_kernels(product_lib, oracle, path):
    """A scene that is one mesh runs the 'flat' kernels (configs 3 and 4), which are compiled without the texture branch; with a
    textured material the host must pick the generic ones - same pixels as the oracle, and a textured G-buffer."""
    pos, faces = scenes.make_torus_knot(64, 16)
    tex = Texture(np.random.default_rng(7).integers(0, 256, (16, 16, 4), dtype=np.uint8))
    s = Scene()
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.15)
    s.Add(Mesh((pos[faces] * np.float32(0.5) + np.float32([0.0, 1.5, -4.0])).astype(np.float32), Material(vec3(0.9, 0.9, 0.9), DiffuseTexture=tex, UVScale=2.0)))
    s.Lights.append(PointLight(vec3(-2.0, 5.0, -1.0), vec3(1, 1, 1), 90.0))
    pose = dict(pos=(0.0, 1.5, 0.5), yaw=0.0, pitch=0.0, fov=55.0)
    o, g = pu.run_pair(oracle, s, 192, 54, 1, pose, frames=2)
    _assert_parity(pu.compare_frame(o, g), "single textured mesh")
    alb = g.read(abi.BUF_G_ALBEDO).reshape(-1, 3)[g.read(abi.BUF_PRIM_ID).reshape(-1) == 0]
    assert len(alb) > 300 and len(np.unique(alb.round(3), axis=0)) > 100
    o.close(); g.close()


@pytest.mark.parametrize("transparent", [False, True])
def test_every_primitive_mirror_and_glass(product_lib, oracle, path, transparent):
    pose = dict(pos=(0.1, 1.2, 1.0), yaw=0.05, pitch=-0.12, fov=50.0)
    o, g = pu.run_pair(oracle, _zoo_scene(transparent), 192, 54, 1, pose, frames=2)
    st = pu.compare_frame(o, g)
    _assert_parity(st, f"zoo transparent={transparent}")
    pid = g.read(abi.BUF_PRIM_ID)
    assert set(np.unique(pid)) >= set(range(0, 7))        # every analytic primitive is seen by some primary ray
    o.close(); g.close()


def test_bunny_full_resolution(product_lib, oracle, path):
    sc, w, h, ss, pose = scenes.config_scene(3)
    o, g = pu.run_pair(oracle, sc, w, h, ss, pose, frames=2, oracle_threads=32)
    _assert_parity(pu.compare_frame(o, g), "cfg3 1280x720")
    assert pu.bits_equal(o.accel(abi.ACCEL_MESH_NODES), g.accel(abi.ACCEL_MESH_NODES))
    assert pu.bits_equal(o.accel(abi.ACCEL_MESH_LEAF_INDEX), g.accel(abi.ACCEL_MESH_LEAF_INDEX))
    o.close(); g.close()


def test_dragon_standin_full_size(product_lib, oracle, path):
    """BASELINE config 4 at its full size: 871,200 triangles, 1920x1080 trace grid."""
    sc, w, h, ss, pose = scenes.config_scene(4)
    o, g = pu.run_pair(oracle, sc, w, h, ss, pose, frames=1, oracle_threads=64)
    _assert_parity(pu.compare_frame(o, g), "cfg4 1920x1080")
    hdr = g.read(abi.BUF_CURRENT_HDR)
    assert np.isfinite(hdr).all() and (hdr >= 0).all()
    o.close(); g.close()


def test_voxel_world_small_and_ss2(product_lib, oracle, path):
    sc, w, h, ss, pose = scenes.config_scene(5, small=True)
    o, g = pu.run_pair(oracle, sc, 160, 45, 2, pose, frames=2)
    _assert_parity(pu.compare_frame(o, g), "cfg5-small ss2")
    o.close(); g.close()


def test_voxel_world_wireframe_close_up(product_lib, oracle, path):
    """Camera a few voxels from a wall so that the fp64 wire test (VolumeGrid.cs:256-283) decides pixels."""
    sc, w, h, ss, pose = scenes.config_scene(5, small=True)
    pose = dict(pose, pitch=-0.9)
    o, g = pu.run_pair(oracle, sc, 128, 36, 1, pose, frames=1)
    st = pu.compare_frame(o, g)
    _assert_parity(st, "cfg5-small close-up")
    alb = g.read(abi.BUF_G_ALBEDO); sky = g.read(abi.BUF_SKY_MASK)
    assert ((alb.sum(-1) == 0) & (sky == 0)).any()        # black wire pixels exist
    o.close(); g.close()


def test_taa_reset_rules_and_resize(product_lib, oracle, path):
    sc, w, h, ss, pose = scenes.config_scene(2)
    o, g = pu.run_pair(oracle, sc, 160, 45, 1, pose, frames=2)
    assert g.stats.history_reset == 0 and o.stats.history_reset == 0
    # move below the threshold (0.0025): no reset; above: reset (TemporalAA.cs:58-67)
    for dx, expect in ((0.001, 0), (0.01, 1)):
        p = (pose["pos"][0] + dx, pose["pos"][1], pose["pos"][2])
        o.set_camera(p, pose["yaw"], pose["pitch"]); g.SetCamera(p, pose["yaw"], pose["pitch"])
        o.render(stages=1, threads=8); g.TryFlipAndBlit()
        assert g.stats.history_reset == expect == o.stats.history_reset
        _assert_parity(pu.compare_frame(o, g), f"taa move {dx}")
        pose = dict(pose, pos=p)
    g.Resize(96, 27, 2)
    assert g.hiW == 192 and g.hiH == 108
    g.TryFlipAndBlit()
    assert g.stats.history_reset == 1 and g.read(abi.BUF_TAA_HISTORY).shape == (108, 192, 3)
    o.close(); g.close()


def test_error_codes(product_lib, path):
    c = abi.default_config()
    ctx = C.c_void_p()
    assert product_lib.ycge_create(C.byref(c), C.byref(ctx)) == 0
    assert product_lib.ycge_render_frame(ctx, None, None) == abi.YCGE_ERR_NO_SCENE          # Scene.cs:73
    assert b"BVH" in product_lib.ycge_last_error(ctx)
    assert product_lib.ycge_scene_upload(ctx, None) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_resize(ctx, 0, 10, 1) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_read_buffer(ctx, abi.BUF_RAYS, C.c_void_p(1), 4) == abi.YCGE_ERR_INVALID_ARG   # needs capture_debug
    empty = flatten(Scene())
    assert product_lib.ycge_scene_upload(ctx, empty.byref()) == 0                            # empty Objects: every ray is sky
    assert product_lib.ycge_render_frame(ctx, None, None) == 0
    product_lib.ycge_destroy(ctx)


@pytest.mark.parametrize("case", ["cornell-2", "cornell-2-lean", "bunny-4"])
def test_two_rank_tile_split_matches_single_gpu(product_lib, path, case, monkeypatch):
    """world_size 2 (4) emulated on one GPU: the contexts trace their tiles, slabs are concatenated as an
    all-gather would, all resolve; results equal the single-context frame bit for bit.  The bunny case splits config 3
    over 4 ranks, whose schedules cut the heavy classes into parts (a rank's default split policy), against a single
    context that does not."""
    lean = case.endswith("lean")             # config.slab_albedo = 0: 8-float slab records, no albedo plane
    floats = tiles.LEAN_SLAB_FLOATS if lean else tiles.SLAB_FLOATS
    if case.startswith("cornell-2"):
        (sc, w, h, ss, pose), world = scenes.config_scene(1), 2
    else:
        (sc, _, _, ss, pose), world = scenes.config_scene(3), 4
        w, h = 320, 90
    flat = flatten(sc)
    import torch
    def mk(rank, world):
        r = RaytraceRenderer(flat, w, h, pose["fov"], ss, rank=rank, world_size=world, slab_albedo=not lean)
        r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        return r
    single = mk(0, 1)
    ranks = [mk(i, world) for i in range(world)]
    nb = ranks[0].tile_slab_bytes()
    assert nb == ranks[1].tile_slab_bytes() == tiles.slab_floats(world, tiles.tile_grid(single.hiW, single.hiH)[2], floats) * 4
    for frame in range(3):
        single.TryFlipAndBlit()
        gathered = torch.zeros(world * nb // 4, dtype=torch.float32, device="cuda")
        for i, r in enumerate(ranks):
            r.trace_tiles(gathered[i * nb // 4:].data_ptr(), 0, want_stats=True)
        torch.cuda.synchronize()
        for r in ranks:
            r.resolve_gathered(gathered.data_ptr(), 0, want_stats=True)
        for which in (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY):
            if lean and which == abi.BUF_G_ALBEDO: continue          # not gathered
            ref = single.read(which)
            for r in ranks:
                assert pu.bits_equal(ref, r.read(which)), (frame, which)
        # the device slab layout is the documented one (tiles.py)
        hdr, alb, nrm = single.read(abi.BUF_CURRENT_HDR), single.read(abi.BUF_G_ALBEDO), single.read(abi.BUF_G_NORMAL)
        full = np.concatenate([hdr, alb, nrm, single.read(abi.BUF_G_DEPTH)[..., None], single.read(abi.BUF_SKY_MASK)[..., None].astype(np.float32)], -1)
        if lean: full = full[..., tiles.LEAN_COLUMNS]
        assert np.array_equal(tiles.unpermute(gathered.cpu().numpy(), single.hiW, single.hiH, world, floats), full)
    if lean:        # the denoise stage needs the albedo plane: refused, not computed from garbage
        with pytest.raises(abi.YcgeError):
            ranks[0].resolve_gathered(gathered.data_ptr(), 0, want_sdr=True)
    for r in ranks + [single]:
        r.close()


def _exchange_halos(ranks, send_bufs, torch):
    """What all_to_all_single does with ycge_halo_counts' split sizes, by device copies: rank q's segment for r lands in r's segment from q."""
    world = len(ranks)
    counts = [r.halo_counts() for r in ranks]
    recv_bufs = [torch.zeros(max(1, sum(counts[r][1])) * 4, dtype=torch.float32, device="cuda") for r in range(world)]
    for q in range(world):
        so = np.concatenate([[0], np.cumsum(counts[q][0])])
        for r in range(world):
            assert counts[q][0][r] == counts[r][1][q], (q, r)
            ro = np.concatenate([[0], np.cumsum(counts[r][1])])
            n = counts[q][0][r]
            if n:
                recv_bufs[r][ro[q] * 4:(ro[q] + n) * 4] = send_bufs[q][so[r] * 4:(so[r] + n) * 4]
    return recv_bufs


@pytest.mark.parametrize("case,world,ring,depth,batch", [("cornell", 2, 0, 1, 0), ("bunny", 4, 4, 3, 0), ("voxel", 3, 3, 2, 0), ("bunny", 8, 6, 5, 0),
                                                         ("bunny", 8, 8, 7, 4), ("bunny", 4, 6, 5, 3), ("cornell", 2, 4, 3, 2), ("voxel", 3, 4, 3, 2)])
@pytest.mark.parametrize("resolve", ["one_launch", "two_launches"])
def test_tile_resident_taa_with_halo_exchange_matches_single_gpu(product_lib, case, world, ring, depth, batch, resolve, monkeypatch):
    """The tile-RESIDENT form (include/ycge.h): every rank traces its tiles, the ranks exchange the one-pixel {hdr, sky} ring of their
    tiles, each runs TAA on its OWN tiles (history resident), the history slabs are gathered.  `world` ranks emulated on one GPU, the
    exchange by device copies with ycge_halo_counts' split sizes; `depth` + 1 traces are issued before the oldest frame is resolved
    (ring of config.tile_ring sets).  The gathered history equals the single-context frame's, bit for bit, over 8 frames of a camera that
    moves below and above the TAA reset thresholds (TemporalAA.cs:58-67) - and so do the halo lists the library hands out and tiles.py's.
    batch > 0: the frames are traced `batch` at a time in ONE launch per rank (ycge_trace_tiles_resident_batch: k_trace_batch for the
    single-launch scenes, frame by frame for the stage pipeline of the voxel world), two batches in flight where the ring has room."""
    import torch
    monkeypatch.delenv("YCGE_PATH", raising=False)
    # the resolve: ONE launch that reads the halo taps from the records where the exchange left them (k_resolve_tiles, round 6, the default) or
    # round 5's two (k_scatter_halo into the planes, then k_taa_tiles)
    if resolve == "two_launches":
        if (case, world, ring) not in (("cornell", 2, 0), ("bunny", 8, 6), ("voxel", 3, 3)): pytest.skip("the two-launch resolve is held on three of the cases")
        monkeypatch.setenv("YCGE_RES_SPLIT_RESOLVE", "1")
    else:
        monkeypatch.delenv("YCGE_RES_SPLIT_RESOLVE", raising=False)
    if case == "cornell":
        sc, w, h, ss, pose = scenes.config_scene(1)
    elif case == "bunny":
        sc, _, _, ss, pose = scenes.config_scene(3); w, h = 320, 90
    else:
        sc, _, _, ss, pose = scenes.config_scene(5, small=True, t01=0.5); w, h = 96, 27
    flat = flatten(sc)
    moves = [0.0, 0.001, 0.0012, 0.02, 0.0201, 0.0201, 0.05, 0.0505]

    def cam(r, i):
        r.SetCamera((pose["pos"][0] + moves[i], pose["pos"][1], pose["pos"][2]), pose["yaw"] + 0.2 * moves[i], pose["pitch"])

    single = RaytraceRenderer(flat, w, h, pose["fov"], ss)
    want, want_reset = [], []
    for i in range(len(moves)):
        cam(single, i)
        single.TryFlipAndBlit()
        want.append(single.read(abi.BUF_TAA_HISTORY)); want_reset.append(int(single.stats.history_reset))
    ranks = [RaytraceRenderer(flat, w, h, pose["fov"], ss, rank=i, world_size=world, tile_ring=ring) for i in range(world)]
    for i, r in enumerate(ranks):          # the library's halo lists are the layout module's
        s_cnt, r_cnt = r.halo_counts()
        send, recv = tiles.halo_lists(i, world, single.hiW, single.hiH)
        assert s_cnt == [len(v) for v in send] and r_cnt == [len(v) for v in recv]
    hb = ranks[0].history_slab_bytes()
    assert hb == tiles.history_slab_floats(world, tiles.tile_grid(single.hiW, single.hiH)[2]) * 4
    n_send = [max(1, sum(r.halo_counts()[0])) for r in ranks]
    pending = []          # (frame index, send buffers) of the traced, unresolved frames
    # with a ring, the traces of consecutive frames go to different streams and the resolves to yet another (bench.py's loop): the library
    # orders a set's trace, exchange, resolve and re-use by its own events, whatever streams the caller brings
    t_streams = [torch.cuda.Stream() for _ in range(ring)] if ring else [None]
    r_stream = torch.cuda.Stream() if ring else None
    sp = lambda st: st.cuda_stream if st is not None else 0

    def resolve_oldest():
        i, send_bufs = pending.pop(0)
        torch.cuda.synchronize()
        recv_bufs = _exchange_halos(ranks, send_bufs, torch)
        gathered = torch.zeros(world * hb // 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()          # (the copies above ran on torch's stream; the resolves below run on a non-blocking one)
        for k, r in enumerate(ranks):
            r.resolve_tiles_resident(recv_bufs[k].data_ptr(), gathered[k * hb // 4:].data_ptr(), sp(r_stream), want_stats=True)
            assert int(r.stats.history_reset) == want_reset[i] and int(r.stats.frame) == i + 1, (i, k)
        torch.cuda.synchronize()
        full = tiles.unpermute(gathered.cpu().numpy(), single.hiW, single.hiH, world, 3)
        assert pu.bits_equal(full, want[i]), f"{case}: gathered history of frame {i + 1} differs"
        ranks[0].unpack_history(gathered.data_ptr(), 0)
        if not pending:          # (reading the consumer's frame joins everything: only where no traced frame waits)
            assert pu.bits_equal(ranks[0].read(abi.BUF_TAA_HISTORY), want[i])

    pose_of = lambda i: ((pose["pos"][0] + moves[i], pose["pos"][1], pose["pos"][2]), pose["yaw"] + 0.2 * moves[i], pose["pitch"], pose["fov"])
    i = 0
    while i < len(moves):
        n = min(batch, len(moves) - i) if batch else 1
        while len(pending) + n > max(depth + 1, n):          # room in the ring for the frames about to be traced
            resolve_oldest()
        frames_bufs = [[torch.zeros(m * 4, dtype=torch.float32, device="cuda") for m in n_send] for _ in range(n)]
        torch.cuda.current_stream().synchronize()
        for k, r in enumerate(ranks):
            if batch:
                r.trace_tiles_resident_batch([pose_of(i + j) for j in range(n)], [frames_bufs[j][k].data_ptr() for j in range(n)], sp(t_streams[(i // n) % len(t_streams)]))
            else:
                cam(r, i)
                r.trace_tiles_resident(frames_bufs[0][k].data_ptr(), sp(t_streams[i % len(t_streams)]))
        for j in range(n):
            pending.append((i + j, frames_bufs[j]))
        i += n
        while len(pending) > depth:
            resolve_oldest()
    while pending:
        resolve_oldest()
    # the ring refuses a trace when every set holds an unresolved frame
    K = ring if ring else 2
    send_bufs = [torch.zeros(n_send[0] * 4, dtype=torch.float32, device="cuda") for _ in range(K + 1)]
    for j in range(K):
        ranks[0].trace_tiles_resident(send_bufs[j].data_ptr(), 0)
    with pytest.raises(abi.YcgeError, match="tile_ring"):
        ranks[0].trace_tiles_resident(send_bufs[K].data_ptr(), 0)
    # ... and so does a batch: more frames than the ring has free sets, more than a launch carries, none
    with pytest.raises(abi.YcgeError, match="tile_ring"):
        ranks[0].trace_tiles_resident_batch([pose_of(0)] * 2, [send_bufs[0].data_ptr()] * 2, 0)
    with pytest.raises(abi.YcgeError, match="1..8"):
        ranks[1].trace_tiles_resident_batch([pose_of(0)] * 9, [send_bufs[0].data_ptr()] * 9, 0)
    with pytest.raises(abi.YcgeError, match="1..8"):
        ranks[1].trace_tiles_resident_batch([], [], 0)
    for r in ranks + [single]:
        r.close()


def test_update_lights_per_frame(product_lib, oracle, path):
    """DayNightEntity-style per-frame light / sky animation through ycge_scene_update_lights."""
    sc, w, h, ss, pose = scenes.config_scene(5, small=True)
    o, g = pu.run_pair(oracle, sc, 96, 27, 1, pose, frames=1)
    lights, top, bottom = scenes.sun_moon_lights(0.31)
    g.UpdateLights(lights, sc.Ambient, top, bottom)
    arr = (abi.Light * len(lights))()
    for i, l in enumerate(lights):
        arr[i].position, arr[i].color, arr[i].intensity = abi.Vec3(*l.Position), abi.Vec3(*l.Color), float(l.Intensity)
    amb, t_, b_ = abi.Vec3(*sc.Ambient.Color), abi.Vec3(*top), abi.Vec3(*bottom)
    assert o.L.orc_scene_update_lights(o.ctx, arr, len(lights), C.byref(amb), float(sc.Ambient.Intensity), C.byref(t_), C.byref(b_)) == 0
    o.render(stages=1, threads=8); g.TryFlipAndBlit()
    _assert_parity(pu.compare_frame(o, g), "lights updated")
    o.close(); g.close()


def _post_pair(oracle, sc, w, h, ss, pose, frames=3):
    """oracle (stages=2) and product (SDR requested) over `frames` frames; yields per-frame comparison tuples"""
    flat = flatten(sc)
    o = oracle.OracleRenderer(sc, w, h, ss, pose, flat=flat)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    out = []
    for f in range(frames):
        so = o.render(stages=2, threads=8, want_sdr=True)
        sg = g.TryFlipAndBlit(want_sdr=True)
        out.append((pu.mismatch_count(o.read(abi.BUF_TAA_HISTORY), g.read(abi.BUF_TAA_HISTORY)),
                    pu.mismatch_count(o.read(abi.BUF_DENOISED), g.read(abi.BUF_DENOISED)),
                    np.float32(o.stats.exposure).view(np.uint32) != np.float32(g.stats.exposure).view(np.uint32),
                    pu.mismatch_count(so, sg), pu.rms(so, sg), float(g.stats.post_ms)))
    o.close(); g.close()
    return out


@pytest.mark.parametrize("cfg_n", [1, 2])
def test_denoise_exposure_tonemap_bit_exact(product_lib, oracle, path, cfg_n):
    """A-trous (incl. the in-place iteration 1), serial auto-exposure sum, box downsample + MapPixel."""
    sc, w, h, ss, pose = scenes.config_scene(cfg_n)
    for f, (taa, den, expo, sdr, sdr_rms, post_ms) in enumerate(_post_pair(oracle, sc, w, h, ss, pose)):
        print(f"cfg{cfg_n} frame {f + 1}: taa {taa} denoised {den} exposure {expo} sdr {sdr} rms {sdr_rms} post_ms {post_ms:.3f}")
        assert taa == 0 and den == 0 and not expo and sdr == 0 and sdr_rms <= pu.RMS_TOL


def test_waived_inplace_iteration_against_the_oracle_and_its_distance_to_the_exact_frame(product_lib, oracle):
    """config.atrous_inplace_exact = 0 ("reproduce or explicitly waive"): iteration 1 of ApplyAtrousDenoise reads A and writes
    B instead of running in place (RaytraceRenderer.cs:718).  The waived form is held to the ORACLE's waived form bit for bit (same
    switch in oracle/orc_render.cpp: only the buffer walk differs), on configs 2 and 3 (a quarter of its size), three frames; and its
    distance to the EXACT frame - what a host gives up for the ~2 ms - is measured here and stated in INTEGRATION.md: RMS over the SDR
    chexel colours (values in [0, 1]) below 5e-3, largest single difference below 0.08."""
    for cfg_n, (w, h) in ((2, (640, 180)), (3, (320, 90))):
        sc, _, _, ss, pose = scenes.config_scene(cfg_n)
        flat = flatten(sc)
        cw = abi.default_config(); cw.atrous_inplace_exact = 0
        co = abi.default_config(); co.atrous_inplace_exact = 0
        o = oracle.OracleRenderer(sc, w, h, ss, pose, flat=flat, cfg=co)
        g = RaytraceRenderer(flat, w, h, pose["fov"], ss, cfg=cw)
        e = RaytraceRenderer(flat, w, h, pose["fov"], ss)
        for r in (g, e):
            r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        for f in range(3):
            so = o.render(stages=2, threads=8, want_sdr=True)
            sg = g.TryFlipAndBlit(want_sdr=True)
            se = e.TryFlipAndBlit(want_sdr=True)
            assert pu.mismatch_count(o.read(abi.BUF_DENOISED), g.read(abi.BUF_DENOISED)) == 0, (cfg_n, f)
            assert np.float32(o.stats.exposure).view(np.uint32) == np.float32(g.stats.exposure).view(np.uint32), (cfg_n, f)
            assert pu.mismatch_count(so, sg) == 0, (cfg_n, f)
            assert pu.bits_equal(g.read(abi.BUF_TAA_HISTORY), e.read(abi.BUF_TAA_HISTORY))          # everything up to TAA is untouched
            d = np.abs(sg.astype(np.float64) - se.astype(np.float64))
            print(f"cfg{cfg_n} frame {f + 1}: waived vs exact SDR rms {np.sqrt((d * d).mean()):.2e} max {d.max():.3f}; post_ms waived {g.stats.post_ms:.3f} exact {e.stats.post_ms:.3f}")
            assert np.sqrt((d * d).mean()) < 5e-3 and d.max() < 0.08
            assert d.max() > 0.0          # (the two forms do differ: the switch is not a no-op)
        o.close(); g.close(); e.close()


@pytest.mark.parametrize("mode", ["0", "2", "3"])
def test_inplace_atrous_in_every_form_against_the_oracle(product_lib, oracle, monkeypatch, mode):
    """The in-place A-trous iteration as ONE persistent launch with level-granular hand-over between the bands' workgroups (0, the
    default; 3: bands in block order) and as a launch per level group (2): the
    denoised frame, the exposure and the SDR frame must equal the oracle's on every frame.  Sizes: several bands (the hand-over is
    exercised), an odd size (border clamps), a width that is not a multiple of a cache line's pixels (two bands share lines)."""
    monkeypatch.setenv("YCGE_POST_MODE", mode)
    sc, _, _, _, pose = scenes.config_scene(2)
    for (w, h, ss) in ((192, 54, 1), (131, 37, 1), (64, 20, 2)):
        for f, (taa, den, expo, sdr, sdr_rms, post_ms) in enumerate(_post_pair(oracle, sc, w, h, ss, pose, frames=3)):
            print(f"mode {mode} {w}x{h} ss{ss} frame {f + 1}: taa {taa} denoised {den} exposure {expo} sdr {sdr}")
            assert taa == 0 and den == 0 and not expo and sdr == 0


def test_post_stage_odd_size_and_supersampling(product_lib, oracle, path):
    """odd trace-grid sizes (border clamps of the in-place schedule) and ss = 2 (box average, exposure step 4)"""
    sc, _, _, _, pose = scenes.config_scene(1)
    for (w, h, ss) in ((37, 19, 1), (21, 13, 2)):
        for f, (taa, den, expo, sdr, sdr_rms, post_ms) in enumerate(_post_pair(oracle, sc, w, h, ss, pose, frames=2)):
            print(f"{w}x{h} ss{ss} frame {f + 1}: taa {taa} denoised {den} exposure {expo} sdr {sdr}")
            assert taa == 0 and den == 0 and not expo and sdr == 0
    sc5, w5, h5, ss5, pose5 = scenes.config_scene(5, small=True)
    for f, (taa, den, expo, sdr, sdr_rms, post_ms) in enumerate(_post_pair(oracle, sc5, 96, 27, 2, pose5, frames=2)):
        assert taa == 0 and den == 0 and not expo and sdr == 0


def test_voxel_world_full_size(product_lib, oracle, path):
    """BASELINE config 5 at its full size: 544x256x544 voxels in 32^3 chunk grids, 3840x2160 trace grid (1080p, ss 2).
    Exercises the persistent extend stage (ray refill) and the HBM part of the traversal stacks at scale."""
    sc, w, h, ss, pose = scenes.config_scene(5)
    o, g = pu.run_pair(oracle, sc, w, h, ss, pose, frames=1, oracle_threads=64)
    _assert_parity(pu.compare_frame(o, g), "cfg5 3840x2160")
    o.close(); g.close()


def test_no_lights_and_single_object(product_lib, oracle, path):
    """degenerate inputs: a scene without lights (no light records are queued) and a one-object scene (BVH = one leaf)"""
    s = _zoo_scene(False)
    s.Lights.clear()
    pose = dict(pos=(0.0, 1.2, 1.5), yaw=0.0, pitch=-0.1, fov=60.0)
    o, g = pu.run_pair(oracle, s, 96, 27, 1, pose, frames=2)
    _assert_parity(pu.compare_frame(o, g), "no lights")
    o.close(); g.close()
    one = Scene()
    one.Add(Sphere(vec3(0.0, 1.0, -3.0), 1.0, Solid(vec3(0.7, 0.3, 0.3))))
    one.Lights.append(PointLight(vec3(2.0, 4.0, 0.0), vec3(1, 1, 1), 40.0))
    o, g = pu.run_pair(oracle, one, 33, 17, 1, dict(pos=(0.0, 1.0, 0.0), yaw=0.0, pitch=0.0, fov=45.0), frames=2)
    _assert_parity(pu.compare_frame(o, g), "one sphere, odd size")
    o.close(); g.close()


def test_update_objects_rebuilds_scene_bvh_only(product_lib, oracle, path):
    """Entity animation (BobbingSphereEntity, TestScenesRandom.cs:708-714 -> Scene.RebuildBVH): the product takes new object
    records through ycge_scene_update_objects, the oracle a full re-upload; frames (and TAA history) must stay identical."""
    def build(dy):
        s = _zoo_scene(False)
        sph = [o for o in s.Objects if isinstance(o, Sphere)][0]
        sph.Center = vec3(sph.Center[0], sph.Center[1] + dy, sph.Center[2])
        return s
    pose = dict(pos=(0.1, 1.2, 1.0), yaw=0.05, pitch=-0.12, fov=50.0)
    o, g = pu.run_pair(oracle, build(0.0), 160, 45, 1, pose, frames=2)
    keep = []
    for step in (1, 2, 3):
        moved = flatten(build(0.15 * step))
        keep.append(moved)
        assert o.L.orc_scene_upload(o.ctx, moved.byref()) == 0
        g.UpdateObjects(moved)
        o.render(stages=1, threads=8); g.TryFlipAndBlit()
        _assert_parity(pu.compare_frame(o, g), f"objects moved, step {step}")
    assert pu.bits_equal(o.accel(abi.ACCEL_SCENE_NODES), g.accel(abi.ACCEL_SCENE_NODES))
    o.close(); g.close()


def test_split_schedule_bit_exact(product_lib, oracle, monkeypatch):
    """YCGE_SPLIT=22222220: the schedule cuts every block above the lowest policy class into 4 parts of 16 pixels, each a k_trace
    wavefront of its own - the same queries in another arrangement: every buffer and every counter must still equal the oracle's.
    Parts need a schedule, i.e. start with the second frame; three frames are compared.  Scenes: the bunny (heavy blocks, diffuse
    bounces), the primitive zoo with glass (path items and transmittance segments), Cornell (not a flat scene: generic walk)."""
    knob = "YCGE_SPLIT=22222220"
    monkeypatch.setenv("YCGE_PATH", "megakernel")
    monkeypatch.setenv("YCGE_SPLIT", "22222220")
    sc3, w3, h3, ss3, pose3 = scenes.config_scene(3)
    sc1, w1, h1, ss1, pose1 = scenes.config_scene(1)
    cases = [("bunny", sc3, 320, 90, 1, pose3), ("zoo+glass", _zoo_scene(True), 192, 54, 1, dict(pos=(0.1, 1.2, 1.0), yaw=0.05, pitch=-0.12, fov=50.0)),
             ("cornell", sc1, w1, h1, ss1, pose1)]
    for label, sc, w, h, ss, pose in cases:
        o, g = pu.run_pair(oracle, sc, w, h, ss, pose, frames=1)
        _assert_parity(pu.compare_frame(o, g), f"{knob} {label} frame1")
        for f in (2, 3):
            o.render(stages=1, threads=8); g.TryFlipAndBlit()
            _assert_parity(pu.compare_frame(o, g), f"{knob} {label} frame{f}")
        o.close(); g.close()


def test_tiled_frame_pipelined_over_two_streams(product_lib, path):
    """bench.py's multi-GPU loop runs the trace of frame N+1 on one stream beside the all-gather + resolve (TAA) of frame N on
    another, with double-buffered slabs: the library keeps the trace's outputs apart from the resolved frame.  One rank in slab
    mode (the gather is a copy): five frames pipelined must equal five frames issued in sequence, bit for bit."""
    import torch
    sc, _, _, ss, pose = scenes.config_scene(3)
    flat = flatten(sc)
    w, h = 320, 90

    def mk():
        r = RaytraceRenderer(flat, w, h, pose["fov"], ss)
        r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        return r
    seq, pip = mk(), mk()
    n = seq.tile_slab_bytes() // 4
    slab = torch.empty(n, dtype=torch.float32, device="cuda")
    for _ in range(5):
        seq.trace_tiles(slab.data_ptr(), 0, want_stats=True)
        seq.resolve_gathered(slab.data_ptr(), 0, want_stats=True)
    slabs = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2)]
    gathered = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2)]
    s_trace, s_comm = torch.cuda.Stream(), torch.cuda.Stream()
    ev_traced = [torch.cuda.Event() for _ in range(2)]
    ev_resolved = [torch.cuda.Event() for _ in range(2)]
    for i in range(5):
        k = i & 1
        with torch.cuda.stream(s_trace):
            s_trace.wait_event(ev_resolved[k])
            pip.trace_tiles(slabs[k].data_ptr(), s_trace.cuda_stream)
            ev_traced[k].record(s_trace)
        with torch.cuda.stream(s_comm):
            s_comm.wait_event(ev_traced[k])
            gathered[k].copy_(slabs[k], non_blocking=True)          # stands in for the all-gather
            pip.resolve_gathered(gathered[k].data_ptr(), s_comm.cuda_stream)
            ev_resolved[k].record(s_comm)
    torch.cuda.synchronize()
    for which in (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY):
        assert pu.bits_equal(seq.read(which), pip.read(which)), which
    seq.close(); pip.close()


def test_empty_scene_and_empty_mesh(product_lib, oracle, path):
    """Edge inputs: Scene.Objects empty (every ray is sky; TAA still runs) matches the oracle frame for frame; a mesh with no
    triangles has no bounds, and the reference's BVH builder refuses such an object ("Unbounded Hittable", BVH.cs) - so do the
    oracle and the product, with the same error."""
    import oracle_binding as ob
    pose = dict(pos=(0.0, 1.0, 0.0), yaw=0.3, pitch=0.1, fov=45.0)
    o, g = pu.run_pair(oracle, Scene(), 64, 20, 1, pose, frames=1)
    _assert_parity(pu.compare_frame(o, g), "empty frame1")
    for f in (2, 3):
        o.render(stages=1, threads=4); g.TryFlipAndBlit()
        _assert_parity(pu.compare_frame(o, g), f"empty frame{f}")
    o.close(); g.close()
    sc = Scene()
    sc.Objects.append(Mesh(np.zeros((0, 3, 3), np.float32), Material(vec3(1, 1, 1))))
    sc.Objects.append(Sphere(vec3(0.0, 1.0, -3.0), 0.7, Material(vec3(0.8, 0.3, 0.2))))
    with pytest.raises(abi.YcgeError, match="Unbounded"):
        ob.OracleRenderer(sc, 64, 20, 1, pose)
    with pytest.raises(abi.YcgeError, match="Unbounded"):
        RaytraceRenderer(sc, 64, 20, pose["fov"], 1)


@pytest.mark.parametrize("fbw,fbh,ss", [(1, 1, 1), (3, 2, 1), (33, 5, 1), (2, 1, 3)])
def test_tiny_and_ragged_framebuffers(product_lib, oracle, path, fbw, fbh, ss):
    """Trace grids smaller than one 32x8 tile / one 8x8 block and ragged at both edges: lanes outside the image must neither
    trace nor write, the schedule has a handful of blocks, TAA's clamp window is all border."""
    sc, _, _, _, pose = scenes.config_scene(2)
    o, g = pu.run_pair(oracle, sc, fbw, fbh, ss, pose, frames=1)
    _assert_parity(pu.compare_frame(o, g), f"{fbw}x{fbh} ss{ss} frame1")
    for f in (2, 3):
        o.render(stages=1, threads=2); g.TryFlipAndBlit()
        _assert_parity(pu.compare_frame(o, g), f"{fbw}x{fbh} ss{ss} frame{f}")
    o.close(); g.close()


def test_more_ranks_than_tiles(product_lib, path):
    """A 33x5 framebuffer is four 32x8 tiles: at world_size 8 half the ranks own nothing.  Their trace and pack are no-ops, their
    slabs are padding, and every rank still resolves the same frame as a single context."""
    import torch
    sc, _, _, _, pose = scenes.config_scene(2)
    flat = flatten(sc)
    w, h, world = 33, 5, 8

    def mk(rank, ws):
        r = RaytraceRenderer(flat, w, h, pose["fov"], 1, rank=rank, world_size=ws)
        r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        return r
    single = mk(0, 1)
    ranks = [mk(i, world) for i in range(world)]
    nb = ranks[0].tile_slab_bytes()
    for frame in range(3):
        single.TryFlipAndBlit()
        gathered = torch.zeros(world * nb // 4, dtype=torch.float32, device="cuda")
        for i, r in enumerate(ranks):
            assert r.tile_slab_bytes() == nb
            r.trace_tiles(gathered[i * nb // 4:].data_ptr(), 0, want_stats=True)
        torch.cuda.synchronize()
        for r in ranks:
            r.resolve_gathered(gathered.data_ptr(), 0, want_stats=True)
        for which in (abi.BUF_CURRENT_HDR, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY):
            ref = single.read(which)
            for r in ranks:
                assert pu.bits_equal(ref, r.read(which)), (frame, which)
    for r in ranks + [single]:
        r.close()


def test_persistent_atrous_when_fewer_band_workgroups_fit(product_lib, monkeypatch):
    """A 3840x2160 trace grid without a sky pixel (config 5's post stage): 540 row-parity half-bands.  The two-set kernel holds
    three band workgroups per CU (768 places), the profiling instantiation two (512): there the host must not take the split layout
    - a band that is not resident while its neighbours wait for it stalls the frame for seconds (measured: 1 - 59 s).  The host asks
    the runtime for the residency of the instantiation it will launch; both builds must produce the same SDR frame, promptly."""
    s = Scene()
    s.Add(Plane(vec3(0.0, 0.0, 0.0), vec3(0.0, 1.0, 0.0), Solid(vec3(0.6, 0.6, 0.55)), 0.05, 0.0))
    s.Add(Sphere(vec3(0.0, 0.5, -2.0), 0.5, Solid(vec3(0.8, 0.2, 0.2))))
    s.Lights.append(PointLight(vec3(1.0, 3.0, -1.0), vec3(1, 1, 1), 30.0))
    out = {}
    # third run: the profiling build made to take the split layout all the same (540 bands, 512 places).  Bands are numbered in order
    # of arrival, so a band's upstream neighbours have always started: slower, never stuck
    for label, probe, assume in (("two-set", None, None), ("profiling", "7", None), ("profiling, 28 bands too many", "7", "3")):
        for k, v in (("YCGE_POST_PROBE_BAND", probe), ("YCGE_POST_ASSUME_RESIDENT", assume)):
            if v is None: monkeypatch.delenv(k, raising=False)
            else: monkeypatch.setenv(k, v)
        r = RaytraceRenderer(s, 1920, 540, 60.0, 2)
        r.SetCamera((0.0, 1.5, 0.0), 0.0, -1.2)         # looking down: ground in every pixel
        frames = []
        for f in range(3):
            frames.append(r.TryFlipAndBlit(want_sdr=True).copy())
            print(f"{label} frame {f + 1}: post {r.stats.post_ms:.2f} ms")
            if f > 0: assert r.stats.post_ms < 200.0, f"{label}: post stage took {r.stats.post_ms:.0f} ms - band workgroups not all resident?"
        assert int(r.read(abi.BUF_SKY_MASK).sum()) == 0
        out[label] = frames
        r.close()
    for other in ("profiling", "profiling, 28 bands too many"):
        for a, b in zip(out["two-set"], out[other]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), other


def test_page_locked_sdr_buffers_of_the_library(product_lib):
    """ABI 8: ycge_alloc_host_buffer hands out page-locked memory of its own (what the C# wrapper's SDR frames live in); ycge_pin_host_buffer
    accepts whole pages the caller owns and nothing else.  The SDR frame written into either kind of memory - by the synchronous call and by
    frames in flight - is the frame an ordinary array receives (RaytraceRenderer.cs:229-264 fills the same chexels either way)."""
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    L = abi.load_library()
    page = L.ycge_host_page_size()
    sc, w, h, ss, pose = scenes.config_scene(2)
    w, h = 96, 27
    n = w * h * 2 * 3
    r = RaytraceRenderer(flatten(sc), w, h, pose["fov"], ss)
    r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    plain = np.zeros(n, dtype=np.float32)
    r._check(L.ycge_render_frame(r.ctx, plain.ctypes.data_as(C.POINTER(C.c_float)), None))
    # (1) the library's own memory
    bufs = []
    for _ in range(3):
        p = C.c_void_p()
        assert L.ycge_alloc_host_buffer(n * 4, C.byref(p)) == abi.YCGE_OK and p.value and p.value % page == 0
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,))
        assert not a.any()
        bufs.append((p, a))
    r2 = RaytraceRenderer(flatten(sc), w, h, pose["fov"], ss)
    r2.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    r2._check(L.ycge_render_frame(r2.ctx, C.cast(bufs[0][0], C.POINTER(C.c_float)), None))
    assert pu.bits_equal(bufs[0][1], plain)
    want = []
    for k in range(3):
        r._check(L.ycge_render_frame(r.ctx, plain.ctypes.data_as(C.POINTER(C.c_float)), None)); want.append(plain.copy())
    for k in range(3):
        r2._check(L.ycge_render_frame_async_sdr(r2.ctx, C.cast(bufs[k][0], C.POINTER(C.c_float))))
    r2.Wait()
    for k in range(3):
        assert pu.bits_equal(bufs[k][1], want[k]), k
    # (2) the caller's own whole pages: accepted, used, released; a range sharing its pages is refused
    span = (n * 4 + page - 1) // page * page
    raw = np.zeros(span + page, dtype=np.uint8)
    off = (-raw.ctypes.data) % page
    mine = raw[off:off + n * 4].view(np.float32)
    assert L.ycge_pin_host_buffer(C.c_void_p(mine.ctypes.data), span) == abi.YCGE_OK
    assert L.ycge_pin_host_buffer(C.c_void_p(mine.ctypes.data + 64), span - page) == abi.YCGE_ERR_INVALID_ARG
    r._check(L.ycge_render_frame(r.ctx, plain.ctypes.data_as(C.POINTER(C.c_float)), None))
    r2._check(L.ycge_render_frame(r2.ctx, mine.ctypes.data_as(C.POINTER(C.c_float)), None))
    assert pu.bits_equal(mine, plain)
    assert L.ycge_unpin_host_buffer(C.c_void_p(mine.ctypes.data)) == abi.YCGE_OK
    r.close(); r2.close()
    # (3) the verdict covers the WHOLE range: a destination that starts inside a page-locked block and runs past its end is
    #     pageable for the library's purposes - staged, or refused by the frames in flight - and so is plain heap memory
    L.ycge_debug_is_page_locked.restype = C.c_int
    L.ycge_debug_is_page_locked.argtypes = [C.c_void_p, C.c_size_t]
    base, nbytes = bufs[0][0].value, n * 4
    assert L.ycge_debug_is_page_locked(C.c_void_p(base), nbytes) == 1
    assert L.ycge_debug_is_page_locked(C.c_void_p(base + 256), nbytes - 512) == 1
    assert L.ycge_debug_is_page_locked(C.c_void_p(base + nbytes - 4096), 64 << 20) == 0, "a range that leaves the block was called page-locked"
    assert L.ycge_debug_is_page_locked(C.c_void_p(plain.ctypes.data), plain.nbytes) == 0
    assert L.ycge_pin_host_buffer(C.c_void_p(mine.ctypes.data), span) == abi.YCGE_OK
    assert L.ycge_debug_is_page_locked(C.c_void_p(mine.ctypes.data), span) == 1
    assert L.ycge_debug_is_page_locked(C.c_void_p(mine.ctypes.data + span - 4096), 2 * 4096 + 4096) == 0 or raw.nbytes >= off + span + 4096
    assert L.ycge_unpin_host_buffer(C.c_void_p(mine.ctypes.data)) == abi.YCGE_OK
    for p, _ in bufs:
        assert L.ycge_free_host_buffer(p) == abi.YCGE_OK
