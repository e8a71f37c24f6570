"""Device chexel colours on the GPU: k_encode_chexels through its hook on inputs a frame never produces, and the frames of
ycge_render_frame_chexels / ycge_render_frame_async_chexels against a twin context driven by ycge_render_frame - the SDR bit for bit, every
encoded byte equal to the restatement (tests/chexel_restatement.py) applied to that SDR."""
import ctypes as C

import numpy as np
import pytest

import chexel_restatement as R
import parity_util as pu
from yetanotherconsolegameengine_amd import abi, build, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
F32 = np.float32
U8P = C.POINTER(C.c_uint8)


def tables(L):
    t32, t64 = np.zeros(255, F32), np.zeros(255, np.float64)
    assert L.ycge_host_srgb_thresholds(t32.ctypes.data_as(C.c_void_p), t64.ctypes.data_as(C.c_void_p)) == 0
    return t32, t64


def hook(g, sdr):
    """k_encode_chexels on an (h, w, 2, 3) f32 array -> (color16, ansi, rgba) as the device computes them"""
    sdr = np.ascontiguousarray(sdr, dtype=F32)
    h, w = sdr.shape[:2]
    c16, ansi, rgba = np.zeros((h, w), np.uint8), np.zeros((h, w, 2), np.uint8), np.zeros((2 * h, w, 4), np.uint8)
    fn = g.L.ycge_test_encode_chexels
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_int32, U8P, U8P, U8P]
    g._check(fn(g.ctx, sdr.ctypes.data_as(C.POINTER(C.c_float)), w, h, c16.ctypes.data_as(U8P), ansi.ctypes.data_as(U8P), rgba.ctypes.data_as(U8P)))
    return c16, ansi, rgba


def assert_encoded(sdr, got, what=""):
    want = R.encode(sdr)
    for name, a, b in zip(("color16", "ansi", "rgba"), got, want):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert bad.size == 0, (what, name, len(bad), bad[:4].tolist())


def as_sdr(values, w):
    """pads a flat f32 vector to whole chexels and lays it out (h, w, 2, 3)"""
    v = np.asarray(values, dtype=F32).ravel()
    per_row = 6 * w
    pad = (-len(v)) % per_row
    v = np.concatenate([v, np.full(pad, 0.5, F32)])
    return v.reshape(-1, w, 2, 3)


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------------------------- 1: the kernel alone
def test_hook_around_every_f32_threshold(enc):
    t32, _ = tables(enc.L)
    bits = (t32.view(np.uint32).astype(np.int64)[:, None] + np.arange(-64, 65)[None, :]).ravel()
    x = np.clip(bits, 0, 0x3F800000).astype(np.uint32).view(F32)
    sdr = as_sdr(x, 97)
    assert_encoded(sdr, hook(enc, sdr), "f32 thresholds")
    # the same values as gray triples, as pairs with their neighbours, in every channel position
    trip = np.stack([x, np.roll(x, 1), np.roll(x, 7)], axis=1)
    for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        sdr = as_sdr(trip[:, perm], 256)
        assert_encoded(sdr, hook(enc, sdr), f"perm {perm}")


def test_hook_gray_triples_around_the_f64_thresholds(enc):
    _, t64 = tables(enc.L)
    # a gray v gives the luminance 0.2126 v + 0.7152 v + 0.0722 v, within an ulp or two of v: binary32 values around each threshold
    # (and unequal triples whose luminance lands there)
    base = t64.astype(F32).view(np.uint32).astype(np.int64)
    v = np.clip((base[:, None] + np.arange(-48, 49)[None, :]).ravel(), 0, 0x3F800000).astype(np.uint32).view(F32)
    gray = np.repeat(v[:, None], 3, axis=1)
    rng = np.random.default_rng(3)
    tilt = (v[:, None] * (1 + rng.uniform(-0.02, 0.02, size=(len(v), 3)))).astype(F32)
    sdr = as_sdr(np.concatenate([gray, tilt]), 128)
    assert_encoded(sdr, hook(enc, sdr), "f64 thresholds")


def test_hook_palette_ties_and_specials(enc):
    vals = [0.0, 0.25, 0.5, 0.625, 0.75, 0.875, 1.0]
    grid = np.array([(a, b, c) for a in vals for b in vals for c in vals], F32)
    sub = np.array([1e-45, 1e-40, 1.1754942e-38, -1e-45], F32)
    sp = np.concatenate([np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, -1.0, 2.0, 1e30, -1e30, 1.0000001, -1e-7,
                                   0.0031308, 0.99999994], F32), sub])
    rng = np.random.default_rng(4)
    mix = rng.choice(np.concatenate([sp, np.array(vals, F32)]), size=(4096, 3)).astype(F32)
    sdr = as_sdr(np.concatenate([grid, mix]), 61)
    got = hook(enc, sdr)
    assert_encoded(sdr, got, "ties and specials")
    assert got[0][0, 0] == 0


def test_hook_sixteen_million_random_values(enc):
    rng = np.random.default_rng(16)
    x = (rng.random(16 * 1024 * 1024, dtype=F32) * F32(1.2) - F32(0.1)).astype(F32)
    sdr = as_sdr(x, 1920)
    assert_encoded(sdr, hook(enc, sdr), "16 M")


@pytest.mark.parametrize("w,h", [(1, 1), (1, 37), (53, 1), (7, 13), (1921, 3)])
def test_hook_odd_shapes(enc, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    sdr = (rng.random((h, w, 2, 3), dtype=F32) * F32(1.4) - F32(0.2)).astype(F32)
    assert_encoded(sdr, hook(enc, sdr), f"{w}x{h}")


# ------------------------------------------------------------------------------------------------------------- 2: frames
FRAME_CASES = [(1, 80, 45, 1), (1, 80, 45, 2), (2, 160, 45, 1), (2, 160, 45, 2), (3, 320, 90, 1), (4, 320, 90, 1), (5, 160, 45, 1)]


def twins(n, w, h, ss, **kw):
    sc, _, _, _, pose = scenes.config_scene(n, small=(n == 5), t01=0.5)
    flat = flatten(sc)
    out = []
    for _ in range(2):
        g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss, **kw)
        g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        out.append(g)
    return out + [pose]


def move(gs, pose, k):
    p = pose["pos"]
    for g in gs:
        g.SetCamera((p[0] + 0.02 * k, p[1], p[2] - 0.01 * k), pose["yaw"] + 0.01 * k, pose["pitch"])


@pytest.mark.parametrize("n,w,h,ss", FRAME_CASES, ids=[f"c{c[0]}-{c[1]}x{c[2]}-ss{c[3]}" for c in FRAME_CASES])
def test_frames_equal_the_plain_frame_and_the_restatement(product_lib, n, w, h, ss):
    a, b, pose = twins(n, w, h, ss)
    try:
        for k in range(3):
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            out = b.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True)
            assert pu.bits_equal(sdr, out["sdr"]), (n, k)
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
            assert_encoded(sdr, (out["color16"], out["ansi"], out["rgba"]), f"config {n} frame {k}")
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def test_each_output_alone_pageable_page_locked_and_interleaved(product_lib):
    a, b, pose = twins(2, 160, 45, 1)
    try:
        forms = [dict(sdr=True, color16=False), dict(color16=True), dict(ansi=True, color16=False), dict(rgba=True, color16=False),
                 "plain", dict(sdr=True, color16=True), "locked", "plain", dict(color16=True, ansi=True, rgba=True, sdr=True)]
        for k, form in enumerate(forms):
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            if form == "plain":
                assert pu.bits_equal(sdr, b.TryFlipAndBlit(want_sdr=True)), k
                continue
            if form == "locked":          # page-locked destinations: the copies go straight into them
                arrs = {name: b._page_locked_zeros(shp, dt)[0] for name, (shp, dt) in b.chexel_shapes().items()}
                b._check(b.L.ycge_render_frame_chexels(b.ctx, *b._chexel_pointers(arrs), None))
                out = {name: arr.copy() for name, arr in arrs.items()}
            else:
                out = b.TryFlipAndBlitChexels(**form)
            want = dict(zip(("color16", "ansi", "rgba"), R.encode(sdr)), sdr=sdr)
            assert out, k
            for name, arr in out.items():
                assert pu.bits_equal(arr, want[name]), (k, name)
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n", [2, 4, 5])
def test_async_sequence_equals_the_sync_sequence(product_lib, n):
    w, h = (320, 90) if n == 4 else (160, 45)
    a, b, pose = twins(n, w, h, 1)
    try:
        sync = []
        for k in range(6):
            move((a,), pose, k)
            sync.append(a.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True))
        got = []
        for k in range(0, 6, 2):          # two frames in flight at a time, one slot each
            move((b,), pose, k)
            o0 = b.RenderAsyncChexels(0, color16=True, ansi=True, rgba=True, sdr=True)
            move((b,), pose, k + 1)
            o1 = b.RenderAsyncChexels(1, color16=True, ansi=True, rgba=True, sdr=True)
            b.Wait()
            got += [{kk: v.copy() for kk, v in o0.items()}, {kk: v.copy() for kk, v in o1.items()}]
        for k, (s, g) in enumerate(zip(sync, got)):
            for name in s:
                assert pu.bits_equal(s[name], g[name]), (n, k, name)
        c16 = b.RenderAsyncChexels(0, color16=True)["color16"]          # one output alone, in flight
        b.Wait()
        assert c16.shape == (h, w)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 3: multi-device forms
def test_peer_push_contexts_on_one_gpu(product_lib):
    a, b, pose = twins(2, 160, 45, 1, devices=[0, 0, 0])
    try:
        for k in range(3):
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            out = b.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True)
            assert pu.bits_equal(sdr, out["sdr"]), k
            assert_encoded(sdr, (out["color16"], out["ansi"], out["rgba"]), f"peer push {k}")
    finally:
        a.close(); b.close()


def _exchange(r):
    mode, world = C.c_int32(-1), C.c_int32(-1)
    r._check(r.L.ycge_exchange_query(r.ctx, C.byref(mode), C.byref(world)))
    return mode.value, world.value


def test_rccl_world_of_one_and_the_lean_slab_refusal(product_lib):
    cfg = abi.default_config()
    cfg.multi_device_exchange = abi.EXCHANGE_RCCL
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    a = RaytraceRenderer(flat, 80, 45, pose["fov"], 1)
    b = RaytraceRenderer(flat, 80, 45, pose["fov"], 1, cfg=cfg, devices=[0])
    try:
        assert _exchange(b) == (abi.EXCHANGE_RCCL, 1), "librccl.so not found or its communicator did not come up"
        for k in range(2):
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            out = b.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True)
            assert pu.bits_equal(sdr, out["sdr"]), k
            assert_encoded(sdr, (out["color16"], out["ansi"], out["rgba"]), f"rccl {k}")
    finally:
        a.close(); b.close()
    cfg = abi.default_config()
    cfg.multi_device_exchange = abi.EXCHANGE_RCCL
    lean = RaytraceRenderer(flat, 80, 45, pose["fov"], 1, cfg=cfg, devices=[0], slab_albedo=False)
    try:
        assert _exchange(lean)[0] == abi.EXCHANGE_RCCL
        c16 = np.zeros((45, 80), np.uint8)
        rc = lean.L.ycge_render_frame_chexels(lean.ctx, None, c16.ctypes.data_as(U8P), None, None, None)
        assert rc == abi.YCGE_ERR_INVALID_ARG and b"lean slabs" in lean.L.ycge_last_error(lean.ctx)
        assert lean.L.ycge_render_frame(lean.ctx, None, None) == abi.YCGE_OK          # (the existing entry is unchanged)
        assert not c16.any()
    finally:
        lean.close()


# ------------------------------------------------------------------------------------------------------------- 4: refusals
def test_refusals_leave_the_context_usable_and_the_arrays_alone(product_lib):
    a, b, pose = twins(1, 80, 45, 1)
    L = b.L
    try:
        assert L.ycge_render_frame_chexels(None, None, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG
        assert L.ycge_render_frame_chexels(b.ctx, None, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG
        assert b"NULL" in L.ycge_last_error(b.ctx)
        assert L.ycge_render_frame_async_chexels(b.ctx, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG
        kept = {name: np.zeros(shp, dt) for name, (shp, dt) in b.chexel_shapes().items()}          # pageable: refused by the async call
        rc = L.ycge_render_frame_async_chexels(b.ctx, *b._chexel_pointers(kept))
        assert rc == abi.YCGE_ERR_INVALID_ARG and b"page-locked" in L.ycge_last_error(b.ctx)
        one = {"color16": kept["color16"]}
        assert L.ycge_render_frame_async_chexels(b.ctx, *b._chexel_pointers(one)) == abi.YCGE_ERR_INVALID_ARG
        for k in range(3):          # the context renders on, its frames equal the twin's (the refusals counted no frame)
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            out = b.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True)
            assert pu.bits_equal(sdr, out["sdr"]), k
            assert_encoded(sdr, (out["color16"], out["ansi"], out["rgba"]), f"after refusals {k}")
            b.RenderAsyncChexels(k % 2, color16=True); b.Wait()
            a.TryFlipAndBlit(want_sdr=True)
        for name, arr in kept.items():
            assert not arr.any(), name
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 5: fault injection
def test_allocation_failure_in_the_first_chexel_call(product_lib):
    """lib/var_faultinject.so: the n-th host allocation of the first _chexels call fails -> YCGE_ERR_OUT_OF_MEMORY; the arrays of a failed
    call are never written afterwards, and the context renders on"""
    L = abi.load_library(build.build_variant("faultinject"))
    L.ycge_debug_fail_allocation.restype = C.c_int
    L.ycge_debug_fail_allocation.argtypes = [C.c_int64]
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    failed, n = 0, 0
    while True:
        g = RaytraceRenderer(flat, w, h, pose["fov"], ss, lib=L)
        try:
            g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
            arrs = {name: np.zeros(shp, dt) for name, (shp, dt) in g.chexel_shapes().items()}
            L.ycge_debug_fail_allocation(n)
            rc = L.ycge_render_frame_chexels(g.ctx, *g._chexel_pointers(arrs), None)
            left = L.ycge_debug_fail_allocation(-1)
            assert rc in (abi.YCGE_OK, abi.YCGE_ERR_OUT_OF_MEMORY), (n, rc, L.ycge_last_error(g.ctx))
            if rc == abi.YCGE_ERR_OUT_OF_MEMORY:
                failed += 1
                assert b"bad_alloc" in L.ycge_last_error(g.ctx)
                for arr in arrs.values():
                    arr[...] = 0          # (what the failed call may have written before it failed is not the question)
                for k in range(2):
                    try:
                        out = g.TryFlipAndBlitChexels(color16=True, ansi=True, rgba=True, sdr=True)
                    except abi.YcgeError as e:
                        raise AssertionError(f"frame {k} after the failure at n = {n}: {e}") from None
                    assert_encoded(out["sdr"], (out["color16"], out["ansi"], out["rgba"]), f"n = {n}, after {k}")
                for name, arr in arrs.items():
                    assert not arr.any(), (n, name)
            else:
                assert_encoded(arrs["sdr"], (arrs["color16"], arrs["ansi"], arrs["rgba"]), f"n = {n}")
                if left >= 0:
                    break
        finally:
            g.close()
        n += 1 if n < 40 else max(1, n // 3)
    assert failed >= 1
