"""-m gpu: what a context leaves behind.  Every GPU resource of the host side is held through the owners of csrc/ycge_own.h, which count
what they hold (ycge_debug_live_resources: device allocations, device bytes, events, streams, page-locked allocations, page-locked bytes,
process-wide).  Each test reads the six counters, runs, and demands the SAME six numbers afterwards - equalities, never bounds; deltas,
because fixtures of the session may hold contexts of their own.  (Page-locked arrays a caller asks for - ycge_alloc_host_buffer - are the
caller's and are not counted.)  No test here provokes a device fault: every call ends in success or in a refusal code."""
import ctypes as C

import numpy as np
import pytest

from yetanotherconsolegameengine_amd import abi, build, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import (AmbientLight, LiveTexture, Material, PointLight, Scene, Sphere, VolumeGrid, XZRect, ZERO, flatten, vec3)

pytestmark = pytest.mark.gpu

NAMES = ("device allocations", "device bytes", "events", "streams", "page-locked allocations", "page-locked bytes")


def live(L):
    out = (C.c_int64 * 6)()
    assert L.ycge_debug_live_resources(out) == abi.YCGE_OK
    return tuple(int(v) for v in out)


def assert_same(L, before, label):
    now = live(L)
    assert now == before, f"{label}: " + ", ".join(f"{n} {b} -> {a}" for n, b, a in zip(NAMES, before, now) if a != b)


def test_create_and_destroy(product_lib):
    L = product_lib
    before = live(L)
    r = RaytraceRenderer(None, 96, 27, lib=L)
    held = live(L)
    assert held[0] > before[0] and held[2] > before[2] and held[3] > before[3], (before, held)          # (the counters do see a context)
    r.close()
    assert_same(L, before, "create / destroy")
    for devices in ([0], [0, 0]):
        RaytraceRenderer(None, 96, 27, lib=L, devices=devices).close()
        assert_same(L, before, f"create / destroy, devices {devices}")


def _query_exchange(r):
    mode, world = C.c_int32(-1), C.c_int32(-1)
    r._check(r.L.ycge_exchange_query(r.ctx, C.byref(mode), C.byref(world)))
    return mode.value, world.value


def _frames_then_destroy(L, devices, exchange, label):
    """create over `devices`, upload, two frames with the post stage, destroy: the counters before and after"""
    sc, w, h, ss, pose = scenes.config_scene(1)
    before = live(L)
    cfg = abi.default_config()
    cfg.multi_device_exchange = exchange
    r = RaytraceRenderer(sc, w, h, pose["fov"], ss, cfg=cfg, devices=devices, lib=L)
    assert _query_exchange(r) == (exchange, len(devices)), f"{label}: the exchange asked for did not come up (librccl.so?)"
    r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    for _ in range(2):
        assert r.TryFlipAndBlit(want_sdr=True).any()
    assert live(L)[0] > before[0]
    r.close()
    assert_same(L, before, label)


def test_rccl_teardown_on_a_world_of_one(product_lib):
    """the teardown order of ~ycge_ctx with a communicator: every rank's streams drained, the communicator destroyed, then the members -
    a world of ONE runs it on a single device (RCCL refuses two ranks on one)"""
    _frames_then_destroy(product_lib, [0], abi.EXCHANGE_RCCL, "RCCL, world of one")


@pytest.mark.parametrize("exchange", [abi.EXCHANGE_PEER_PUSH, abi.EXCHANGE_RCCL], ids=["peer_push", "rccl"])
def test_teardown_over_two_real_devices(product_lib, exchange):
    """peers on OTHER devices: their workers stopped, their streams drained with their device current, the communicators destroyed, the
    peers deleted, in that order - skipped on a box with one device, as tests/test_gpu_timed_variants.py's two-device case is"""
    n = product_lib.ycge_device_count()
    if n < 2:
        pytest.skip(f"needs >= 2 HIP devices; this box has {n}")
    _frames_then_destroy(product_lib, [0, 1], exchange, f"two devices, exchange {exchange}")


def _busy_scene():
    """analytic objects, a live texture, and materials a streamed grid may name"""
    rng = np.random.default_rng(3)
    tex = LiveTexture(rng.integers(0, 256, (24, 32, 3), dtype=np.uint8))
    mats = [Material(vec3(*rng.uniform(0.1, 0.9, 3)), 0.1, 0.0, ZERO) for _ in range(4)]
    s = Scene()
    s.HasDynamicTextures = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.1)
    s.Add(XZRect(-6.0, 6.0, -12.0, 2.0, 0.0, Material(vec3(0.8, 0.8, 0.8), DiffuseTexture=tex, UVScale=2.0), 0.05, 0.0))
    for k, m in enumerate(mats):
        s.Add(Sphere(vec3(-1.5 + k, 0.5, -4.0), 0.5, m))
    s.Lights.append(PointLight(vec3(-2.0, 5.0, -1.0), vec3(1.0, 0.95, 0.9), 90.0))
    s.BackgroundTop, s.BackgroundBottom = vec3(0.5, 0.7, 1.0), vec3(0.9, 0.95, 1.0)
    cells = np.zeros((9, 8, 7, 2), np.int32)
    cells[2:6, 1:5, 2:5, 0] = rng.integers(1, 4, (4, 4, 3))
    grid = VolumeGrid(cells, vec3(2.0, 0.0, -6.0), vec3(0.25, 0.25, 0.25), lambda a, b: mats[(a + b) % len(mats)])
    return s, tex, grid, rng


def test_a_context_that_did_everything_leaves_nothing(product_lib):
    """upload, a synchronous SDR frame into a pageable array, frames in flight without and with the post stage, a _chexels and an _ansi
    frame, a scene query, a live texture's next frame, an attach and a detach of a grid - then destroy"""
    L = product_lib
    before = live(L)
    s, tex, grid, rng = _busy_scene()
    r = RaytraceRenderer(s, 96, 27, 55.0, 2, lib=L)
    r.SetCamera((0.2, 1.7, 2.2), 0.04, -0.22)
    sdr = np.zeros((r.fbH, r.fbW, 2, 3), np.float32)          # (pageable: the staged read-back)
    r._check(L.ycge_render_frame(r.ctx, sdr.ctypes.data_as(C.POINTER(C.c_float)), None))
    assert sdr.any()
    for _ in range(4):
        r.RenderAsync()
    r.Wait()
    slots = [r.RenderAsync(sdr_slot=k % 3) for k in range(5)]
    r.Wait()
    assert slots[-1].any()
    out = r.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True)
    assert out["rgba"].any()
    assert len(r.TryFlipAndBlitAnsi(r.fbW, r.fbH, clear_screen=True)) > 0
    o = np.float32([[0.0, 3.0, -4.0]]); d = np.float32([[0.0, -1.0, 0.0]])
    r.Hit(o, d); assert r.Occluded(o, d).shape == (1,)
    tex.set_frame(rng.integers(0, 256, tex.frame.shape, dtype=np.uint8)); r.UpdateTexture(tex)
    r.TryFlipAndBlit()
    idx = r.AttachGrids([grid])
    r.TryFlipAndBlit()
    r.DetachGrids(idx)
    r.TryFlipAndBlit(want_sdr=True)
    held = live(L)
    assert held[4] > before[4], (before, held)          # (the staging the calls above made is counted)
    r.close()
    assert_same(L, before, "a context that did everything")


def _resident_frames(r, torch, frames=3):
    """the tile-resident form on a world of one: no halo records travel, the history slab is the whole frame's"""
    hist = torch.zeros(max(4, r.history_slab_bytes() // 4), dtype=torch.float32, device="cuda")
    halo = torch.zeros(16, dtype=torch.float32, device="cuda")
    for _ in range(frames):
        r.trace_tiles_resident(halo.data_ptr(), 0)
        r.resolve_tiles_resident(halo.data_ptr(), hist.data_ptr(), 0)
    torch.cuda.synchronize()
    assert bool(hist.abs().sum() > 0)


def test_the_resident_ring_goes_with_every_resize(product_lib):
    """ycge_trace_tiles_resident + ycge_resolve_tiles_resident, ycge_resize, the same calls again - twice - then destroy.  After each
    resize the context holds on the device exactly what a fresh context of that size holds after the same calls.  (The sizes GROW: the
    one buffer that is kept across a resize when the new contents fit - the tile table, DevBuf::upload - is then allocated anew each time,
    so "a fresh context" is the right yardstick to the byte.)"""
    import torch
    L = product_lib
    sc, _, _, _, pose = scenes.config_scene(1)
    flat = flatten(sc)
    sizes = [(80, 45, 1), (96, 54, 1), (80, 45, 2)]
    before = live(L)

    def fresh(size):
        r = RaytraceRenderer(flat, size[0], size[1], pose["fov"], size[2], lib=L)
        r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        _resident_frames(r, torch)
        held = live(L)
        r.close()
        assert_same(L, before, f"a fresh context of {size}")
        return tuple(h - b for h, b in zip(held, before))

    want = [fresh(s) for s in sizes]
    r = RaytraceRenderer(flat, *sizes[0][:2], pose["fov"], sizes[0][2], lib=L)
    r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    _resident_frames(r, torch)
    for size, w in zip(sizes[1:], want[1:]):
        r.Resize(*size)
        _resident_frames(r, torch)
        held = tuple(h - b for h, b in zip(live(L), before))
        print(f"resident ring after ycge_resize to {size}: holds {held[1]} device bytes in {held[0]} allocations; a fresh context {w[1]} in {w[0]}")
        assert held[:2] == w[:2], f"after ycge_resize to {size}: {held[1] - w[1]} device bytes ({held[0] - w[0]} allocations) more than a fresh context of that size"
    r.close()
    assert_same(L, before, "resident form, two resizes")


def test_the_resident_loop_hook_frees_what_it_makes(product_lib):
    L = product_lib
    L.ycge_debug_resident_loop.restype = C.c_int
    L.ycge_debug_resident_loop.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    sc, w, h, ss, pose = scenes.config_scene(1)
    r = RaytraceRenderer(sc, w, h, pose["fov"], ss, lib=L, tile_ring=3)
    r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    period, issue = C.c_double(), C.c_double()
    r._check(L.ycge_debug_resident_loop(r.ctx, 1, C.byref(period), C.byref(issue)))          # (the first call makes the ring: the context's, kept)
    before = live(L)
    r._check(L.ycge_debug_resident_loop(r.ctx, 8, C.byref(period), C.byref(issue)))
    assert period.value > 0.0
    assert_same(L, before, "ycge_debug_resident_loop")
    r.close()


@pytest.mark.parametrize("entry", ["ycge_render_frame", "ycge_render_frame_chexels", "ycge_render_frame_ansi"])
def test_a_failed_frame_leaves_no_latched_sdr_destination(entry):
    """lib/var_faultinject.so: the n-th host allocation of a context's FIRST frame with the post stage, into PAGEABLE arrays - the SDR array, and
    with it a console-16 array (_chexels) or an out_stream of ycge_ansi_stream_bound bytes (_ansi) - fails.  After every step that returned an
    error the arrays are filled with a pattern and one successful frame is rendered with out_sdr = NULL: the patterns are intact (no pointer of
    the failed call outlived it), that frame - no post stage - changed no counter, and the context's destruction gives everything back.  The
    guarantee is structural: a call's destinations, staged ones included, are a value on its entry point's stack that is passed down to the post
    stage, and the context has no member that could hold one - the walk checks that nothing else took the place of the latch it once had."""
    L = abi.load_library(build.build_variant("faultinject"))
    L.ycge_debug_fail_allocation.restype = C.c_int
    L.ycge_debug_fail_allocation.argtypes = [C.c_int64]
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    before = live(L)
    failed, n = 0, 0
    while True:
        g = RaytraceRenderer(flat, w, h, pose["fov"], ss, lib=L)
        try:
            g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
            sdr = np.zeros((g.fbH, g.fbW, 2, 3), np.float32)
            bound = C.c_size_t(0)
            assert L.ycge_ansi_stream_bound(g.fbW, g.fbH, C.byref(bound)) == abi.YCGE_OK
            c16 = np.zeros(bound.value if entry == "ycge_render_frame_ansi" else (g.fbH, g.fbW), np.uint8)          # (_ansi: the stream's bytes)
            p_sdr, p_c16 = sdr.ctypes.data_as(C.POINTER(C.c_float)), c16.ctypes.data_as(C.POINTER(C.c_uint8))
            assert L.ycge_render_frame(g.ctx, None, None) == abi.YCGE_OK          # (what a trace-only frame makes on first use exists from here on)
            L.ycge_debug_fail_allocation(n)
            if entry == "ycge_render_frame":
                rc = L.ycge_render_frame(g.ctx, p_sdr, None)
            elif entry == "ycge_render_frame_chexels":
                rc = L.ycge_render_frame_chexels(g.ctx, p_sdr, p_c16, None, None, None)
            else:
                rc = L.ycge_render_frame_ansi(g.ctx, g.fbW, g.fbH, 0, 0, 7, 0, 0, p_c16, bound.value, C.byref(C.c_size_t(0)), p_sdr, None)
            left = L.ycge_debug_fail_allocation(-1)
            assert rc in (abi.YCGE_OK, abi.YCGE_ERR_OUT_OF_MEMORY), (n, rc, L.ycge_last_error(g.ctx))
            if rc == abi.YCGE_ERR_OUT_OF_MEMORY:
                failed += 1
                sdr[...] = np.float32(-7.5); c16[...] = 0xA5
                held = live(L)
                assert L.ycge_render_frame(g.ctx, None, None) == abi.YCGE_OK, (n, L.ycge_last_error(g.ctx))
                assert (sdr == np.float32(-7.5)).all() and (c16 == 0xA5).all(), f"n = {n}: a later frame wrote into an array of the failed call"
                assert_same(L, held, f"n = {n}: the frame after the failure")
            else:
                assert sdr.any()
        finally:
            g.close()
        assert_same(L, before, f"n = {n}: after ycge_destroy")
        if rc == abi.YCGE_OK and left >= 0:
            break
        n += 1 if n < 40 else max(1, n // 3)
    print(f"{entry}: {failed} of the walk's steps failed (up to n = {n})")
    assert failed >= 1, failed
