"""The ANSI escape stream on the GPU: the stream kernels through their hook (ycge_test_ansi_stream) on pairs a frame never produces, and
the frames of ycge_render_frame_ansi against the restatement (tests/ansi_stream_restatement.py) of the SDR the same call returned, that
SDR against a twin context driven by ycge_render_frame.  Every stream is compared byte for byte, with its exact length and a canary
behind it."""
import ctypes as C

import numpy as np
import pytest

import ansi_stream_restatement as A
import parity_util as pu
from yetanotherconsolegameengine_amd import abi, build, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
U8P = C.POINTER(C.c_uint8)
CANARY = 0xA5


def hook(g, pairs, cw, ch, viewport=(0, 0), fg=7, bg=0, clear=False):
    """ycge_test_ansi_stream on (fbH, fbW, 2) pairs -> the stream; checks that nothing past its length was written"""
    pairs = np.ascontiguousarray(pairs, dtype=np.uint8)
    fbH, fbW = pairs.shape[:2]
    cap = RaytraceRenderer.ansi_stream_bound(cw, ch, g.L)
    out = np.full(cap + 64, CANARY, np.uint8)
    n = C.c_size_t(0)
    fn = g.L.ycge_test_ansi_stream
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, U8P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                   U8P, C.c_size_t, C.POINTER(C.c_size_t)]
    g._check(fn(g.ctx, pairs.ctypes.data_as(U8P), fbW, fbH, cw, ch, viewport[0], viewport[1], fg, bg, int(clear), out.ctypes.data_as(U8P), cap, C.byref(n)))
    assert n.value <= cap
    assert (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes()


def first_difference(a, b):
    n = min(len(a), len(b))
    k = next((i for i in range(n) if a[i] != b[i]), n)
    return k, a[max(0, k - 24):k + 24], b[max(0, k - 24):k + 24]


def assert_stream(got, want, what=""):
    assert len(got) == len(want) and got == want, (what, len(got), len(want), first_difference(got, want))


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------------------------- 1: the kernels alone
def _pattern(kind, h, w):
    k = np.arange(h * w).reshape(h, w)
    p = np.zeros((h, w, 2), np.uint8)
    if kind == "equal":
        p[...] = (100, 200)
    elif kind == "fg":
        p[..., 0], p[..., 1] = k % 256, 7
    elif kind == "bg":
        p[..., 0], p[..., 1] = 7, k % 256
    else:
        p[..., 0], p[..., 1] = k % 256, (k + 1) % 256
    return p


@pytest.mark.parametrize("kind", ["equal", "fg", "bg", "both"])
@pytest.mark.parametrize("w,h", [(7, 3), (1100, 3), (33, 70)])
def test_hook_escape_branches(enc, kind, w, h):
    p = _pattern(kind, h, w)
    for clear in (False, True):
        assert_stream(hook(enc, p, w, h, clear=clear), A.stream(p, w, h, clear=clear), (kind, w, h, clear))


def test_hook_index_digits(enc):
    vals = np.array([0, 9, 10, 99, 100, 255], np.uint8)
    a, b = np.meshgrid(vals, vals, indexing="ij")
    pairs = np.stack([a.ravel(), b.ravel()], axis=1)
    p = np.concatenate([pairs, pairs[::-1], pairs[::3], pairs[1::2]]).reshape(-1, 17, 2)
    h, w = p.shape[:2]
    for fg, bg in [(0, 0), (7, 0), (15, 8), (3, 12)]:
        assert_stream(hook(enc, p, w + 2, h + 1, (1, 0), fg, bg), A.stream(p, w + 2, h + 1, (1, 0), fg, bg), (fg, bg))


def test_hook_four_digit_rows(enc):
    rng = np.random.default_rng(1001)
    p = rng.integers(0, 4, (1001, 3, 2)).astype(np.uint8)
    assert_stream(hook(enc, p, 3, 1001), A.stream(p, 3, 1001), "3 x 1001")
    assert b"\x1b[1000;1H" in A.stream(p, 3, 1001) and b"\x1b[1001;1H" in A.stream(p, 3, 1001)


@pytest.mark.parametrize("cw,ch,vp", [(31, 17, (0, 0)), (31, 17, (5, 3)), (31, 17, (-4, -2)), (31, 17, (-20, 2)), (31, 17, (40, 0)),
                                      (31, 17, (0, 30)), (31, 17, (-100, -100)), (12, 10, (0, 0)), (1, 1, (0, 0)), (1, 1, (1, 0)),
                                      (1, 1, (-19, -9)), (21, 11, (0, 0))])
def test_hook_geometry(enc, cw, ch, vp):
    rng = np.random.default_rng(abs(cw * 100 + ch + 7 * vp[0] + vp[1]))
    p = rng.integers(0, 256, (11, 20, 2)).astype(np.uint8)
    p[2:5, 3:9] = (44, 45)                      # runs of equal cells
    assert_stream(hook(enc, p, cw, ch, vp, 2, 14, clear=True), A.stream(p, cw, ch, vp, 2, 14, clear=True), (cw, ch, vp))


def test_hook_one_by_one_framebuffer(enc):
    p = np.array([[[255, 0]]], np.uint8)
    for cw, ch, vp in [(1, 1, (0, 0)), (3, 2, (1, 1)), (3, 2, (5, 5))]:
        assert_stream(hook(enc, p, cw, ch, vp), A.stream(p, cw, ch, vp), (cw, ch, vp))


def test_hook_random_pairs_1920x540(enc):
    rng = np.random.default_rng(540)
    p = rng.integers(0, 256, (540, 1920, 2)).astype(np.uint8)
    p[:, 100:400] = p[:, 100:101]               # long runs of equal cells too
    assert_stream(hook(enc, p, 1921, 541, clear=True), A.stream(p, 1921, 541, clear=True), "1920x540 in 1921x541")


# ------------------------------------------------------------------------------------------------------------- 2: frames
FRAME_CASES = [(1, 80, 45, 1), (2, 160, 45, 1), (2, 160, 45, 2), (3, 320, 90, 1), (4, 320, 90, 1), (5, 160, 45, 1)]


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
        geometries = [(w + 1, h + 1, (0, 0), 7, 0, True), (w + 1, h, (0, 0), 7, 0, False), (w, h, (0, 0), 15, 1, False)]
        for k, (cw, ch, vp, fg, bg, clear) in enumerate(geometries):          # the second: the product's (framebuffer one column narrower)
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, s2 = b.TryFlipAndBlitAnsi(cw, ch, vp, fg, bg, clear, sdr=True)
            assert pu.bits_equal(sdr, s2), (n, k)
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
            assert_stream(stream, A.frame_stream(s2, cw, ch, vp, fg, bg, clear), f"config {n} frame {k}")
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def test_resize_clear_toggling_and_interleaved_forms(product_lib):
    a, b, pose = twins(2, 160, 45, 1)
    try:
        plan = [(160, 45, True), (160, 45, False), "plain", (96, 30, True), (96, 30, False), "chexels", (200, 60, False), (200, 60, True)]
        size = (160, 45)
        for k, step in enumerate(plan):
            move((a, b), pose, k)
            if step not in ("plain", "chexels") and step[:2] != size:
                size = step[:2]
                a.Resize(size[0], size[1], 1); b.Resize(size[0], size[1], 1)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            if step == "plain":
                assert pu.bits_equal(sdr, b.TryFlipAndBlit(want_sdr=True)), k
                continue
            if step == "chexels":
                out = b.TryFlipAndBlitChexels(ansi=True, color16=False, sdr=True)
                assert pu.bits_equal(sdr, out["sdr"]), k
                continue
            fbW, fbH, clear = step
            stream, s2 = b.TryFlipAndBlitAnsi(fbW + 1, fbH, clear_screen=clear, sdr=True)
            assert pu.bits_equal(sdr, s2), k
            assert_stream(stream, A.frame_stream(s2, fbW + 1, fbH, clear=clear), f"step {k}")
            assert stream.startswith(b"\x1b[2J\x1b[H") == clear
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def _call(g, cw, ch, out, cap, n, sdr=None, fg=7, bg=0, vp=(0, 0), clear=0, stats=None):
    return g.L.ycge_render_frame_ansi(g.ctx, cw, ch, vp[0], vp[1], fg, bg, clear, out.ctypes.data_as(U8P) if out is not None else None, cap,
                                      C.byref(n) if n is not None else None, sdr.ctypes.data_as(C.POINTER(C.c_float)) if sdr is not None else None,
                                      stats)


def test_pageable_and_page_locked_destinations(product_lib):
    a, b, pose = twins(1, 80, 45, 1)
    try:
        cw, ch = 81, 45
        cap = RaytraceRenderer.ansi_stream_bound(cw, ch, b.L)
        for k, form in enumerate(["pageable", "locked", "pageable", "locked"]):
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            if form == "locked":
                out = b._page_locked_zeros((cap + 64,), np.uint8)[0]
                s2 = b._page_locked_zeros((45, 80, 2, 3))[0]
            else:
                out, s2 = np.zeros(cap + 64, np.uint8), np.zeros((45, 80, 2, 3), np.float32)
            out[...] = CANARY
            n = C.c_size_t(0)
            b._check(_call(b, cw, ch, out, cap, n, s2))
            assert pu.bits_equal(sdr, s2), k
            assert (out[n.value:] == CANARY).all(), k
            assert_stream(out[:n.value].tobytes(), A.frame_stream(s2, cw, ch), f"{form} {k}")
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 3: multi-device forms
def test_peer_push_contexts_on_one_gpu(product_lib):
    a, b, pose = twins(2, 160, 45, 1, devices=[0, 0, 0])
    try:
        for k in range(3):
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, s2 = b.TryFlipAndBlitAnsi(161, 45, sdr=True, clear_screen=(k == 0))
            assert pu.bits_equal(sdr, s2), k
            assert_stream(stream, A.frame_stream(s2, 161, 45, clear=(k == 0)), f"peer push {k}")
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
            stream, s2 = b.TryFlipAndBlitAnsi(81, 45, sdr=True)
            assert pu.bits_equal(sdr, s2), k
            assert_stream(stream, A.frame_stream(s2, 81, 45), f"rccl {k}")
    finally:
        a.close(); b.close()
    cfg = abi.default_config()
    cfg.multi_device_exchange = abi.EXCHANGE_RCCL
    lean = RaytraceRenderer(flat, 80, 45, pose["fov"], 1, cfg=cfg, devices=[0], slab_albedo=False)
    try:
        assert _exchange(lean)[0] == abi.EXCHANGE_RCCL
        cap = RaytraceRenderer.ansi_stream_bound(81, 45, lean.L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        rc = _call(lean, 81, 45, out, cap, n)
        assert rc == abi.YCGE_ERR_INVALID_ARG and b"lean slabs" in lean.L.ycge_last_error(lean.ctx)
        assert lean.L.ycge_render_frame(lean.ctx, None, None) == abi.YCGE_OK          # (the existing entry is unchanged)
        assert not out.any() and n.value == 0
    finally:
        lean.close()


# ------------------------------------------------------------------------------------------------------------- 4: refusals
def test_refusals_leave_the_context_usable_and_the_arrays_alone(product_lib):
    a, b, pose = twins(1, 80, 45, 1)
    L = b.L
    try:
        cap = RaytraceRenderer.ansi_stream_bound(81, 45, L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        s2 = np.zeros((45, 80, 2, 3), np.float32)
        assert L.ycge_render_frame_ansi(None, 81, 45, 0, 0, 7, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), None, None) == abi.YCGE_ERR_INVALID_ARG
        refusals = [
            (dict(cw=81, ch=45, out=out, cap=cap - 1, n=n), [b"capacity %d" % (cap - 1), b"bound %d" % cap]),
            (dict(cw=81, ch=45, out=None, cap=cap, n=n), [b"NULL"]),
            (dict(cw=81, ch=45, out=out, cap=cap, n=None), [b"NULL"]),
            (dict(cw=0, ch=45, out=out, cap=cap, n=n), [b"positive"]),
            (dict(cw=81, ch=-1, out=out, cap=cap, n=n), [b"positive"]),
            (dict(cw=81, ch=45, out=out, cap=cap, n=n, fg=16), [b"0..15"]),
            (dict(cw=81, ch=45, out=out, cap=cap, n=n, bg=-1), [b"0..15"]),
            (dict(cw=100000, ch=2000, out=out, cap=cap, n=n), [b"2^32"]),
        ]
        for kw, words in refusals:
            rc = _call(b, sdr=s2, **kw)
            msg = L.ycge_last_error(b.ctx)
            assert rc == abi.YCGE_ERR_INVALID_ARG, (kw, rc, msg)
            for wd in words:
                assert wd in msg, (kw, msg)
        for k in range(3):          # the context renders on, its frames equal the twin's (the refusals counted no frame)
            move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, got = b.TryFlipAndBlitAnsi(81, 45, sdr=True)
            assert pu.bits_equal(sdr, got), k
            assert a.stats.frame == b.stats.frame, k
            assert_stream(stream, A.frame_stream(got, 81, 45), f"after refusals {k}")
        assert not out.any() and not s2.any() and n.value == 0
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 5: fault injection
def test_allocation_failure_in_the_first_ansi_call(product_lib):
    """lib/var_faultinject.so: the n-th host allocation of the first _ansi call fails -> YCGE_ERR_OUT_OF_MEMORY; the arrays of a failed
    call are never written afterwards, and the context renders on"""
    L = abi.load_library(build.build_variant("faultinject"))
    L.ycge_debug_fail_allocation.restype = C.c_int
    L.ycge_debug_fail_allocation.argtypes = [C.c_int64]
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    cw, ch = w + 1, h
    failed, n = 0, 0
    while True:
        g = RaytraceRenderer(flat, w, h, pose["fov"], ss, lib=L)
        try:
            g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
            cap = RaytraceRenderer.ansi_stream_bound(cw, ch, L)
            out, ln, s2 = np.zeros(cap, np.uint8), C.c_size_t(0), np.zeros((h, w, 2, 3), np.float32)
            L.ycge_debug_fail_allocation(n)
            rc = _call(g, cw, ch, out, cap, ln, s2)
            left = L.ycge_debug_fail_allocation(-1)
            assert rc in (abi.YCGE_OK, abi.YCGE_ERR_OUT_OF_MEMORY), (n, rc, L.ycge_last_error(g.ctx))
            if rc == abi.YCGE_ERR_OUT_OF_MEMORY:
                failed += 1
                assert b"bad_alloc" in L.ycge_last_error(g.ctx)
                assert ln.value == 0, n
                out[...] = 0; s2[...] = 0          # (what the failed call may have written before it failed is not the question)
                for k in range(2):
                    try:
                        stream, got = g.TryFlipAndBlitAnsi(cw, ch, sdr=True)
                    except abi.YcgeError as e:
                        raise AssertionError(f"frame {k} after the failure at n = {n}: {e}") from None
                    assert_stream(stream, A.frame_stream(got, cw, ch), f"n = {n}, after {k}")
                assert not out.any() and not s2.any(), n
            else:
                assert_stream(out[:ln.value].tobytes(), A.frame_stream(s2, cw, ch), f"n = {n}")
                if left >= 0:
                    break
        finally:
            g.close()
        n += 1 if n < 40 else max(1, n // 3)
    assert failed >= 1
