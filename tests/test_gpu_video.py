"""Video mode on the GPU: ycge_video_blit / ycge_video_blit_ansi and the kernel's hook against the restatement of Renderer/VideoRenderer.cs
(tests/video_restatement.py).  Every comparison is bitwise; nothing in this path can produce a NaN."""
import ctypes as C

import numpy as np
import pytest

import ansi_stream_restatement as A
import chexel_restatement as CR
import parity_util as pu
import video_restatement as VR
from yetanotherconsolegameengine_amd import abi, build, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VideoRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
U8P = C.POINTER(C.c_uint8)
CANARY = 0xA5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_sdr(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    assert not np.isnan(got).any()


def make_frame(kind, h, w, bpp, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        f = rng.integers(0, 256, (h, w, bpp), dtype=np.uint8)
    elif kind == "zeros":
        f = np.zeros((h, w, bpp), np.uint8)
    elif kind == "ones":
        f = np.full((h, w, bpp), 255, np.uint8)          # Lanczos overshoot: accumulators above 1, Clamp01
    elif kind == "checker":
        f = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)[..., None].repeat(bpp, 2)
    elif kind == "hramp":
        f = np.broadcast_to((np.arange(w) * 255 // max(1, w - 1)).astype(np.uint8)[None, :, None], (h, w, bpp))
    else:
        f = np.broadcast_to((np.arange(h) * 255 // max(1, h - 1)).astype(np.uint8)[:, None, None], (h, w, bpp))
    f = np.ascontiguousarray(f)
    if bpp == 4:
        f[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)          # the 4th byte is ignored
    return f


@pytest.fixture(scope="module")
def vid(product_lib):
    v = VideoRenderer(8, 4, 1, lib=product_lib)          # no scene, ever
    yield v
    v.close()


# (src_w, src_h, fbW, fbH, ss): sources smaller and larger than the grid, letterboxed in x and in y, 1 x 1 / 1 x N / N x 1 sources, odd and 1 x 1
# framebuffers, ss 1..4
HOOK_CASES = [(16, 12, 11, 5, 1), (16, 12, 11, 5, 2), (16, 12, 7, 9, 3), (16, 12, 5, 3, 4), (64, 48, 13, 3, 1), (64, 48, 3, 11, 2), (200, 150, 9, 7, 1), (5, 4, 40, 20, 1),
              (5, 4, 33, 9, 2), (1, 1, 4, 3, 1), (1, 1, 1, 1, 3), (1, 9, 6, 5, 2), (9, 1, 6, 5, 1), (31, 17, 1, 1, 1), (31, 17, 1, 1, 4), (640, 480, 237, 62, 2), (1280, 720, 120, 40, 4),
              (3, 2, 7, 5, 3), (130, 70, 65, 35, 1), (129, 3, 70, 2, 1)]


@pytest.mark.parametrize("case", HOOK_CASES, ids=["%dx%d-%dx%d-ss%d" % c for c in HOOK_CASES])
def test_kernel_equals_the_restatement(vid, case):
    sw, sh, fw, fh, ss = case
    kinds = ["random", "ones", "checker"] if sw * sh > 100000 else ["random", "zeros", "ones", "checker", "hramp", "vramp"]
    for kind in kinds:
        f3 = make_frame(kind, sh, sw, 3, seed=sw + fh)
        f4 = make_frame(kind, sh, sw, 4, seed=sw + fh)
        f4[..., :3] = f3
        want = VR.blit(f3, sw, sh, 3, fw, fh, ss)
        got3 = vid.blit_probe(f3, fw, fh, ss)
        got4 = vid.blit_probe(f4, fw, fh, ss)
        assert_sdr(got3, want, f"{case} {kind} bgr")
        assert_sdr(got4, want, f"{case} {kind} bgra")
        if kind == "zeros":
            assert not got3.any()


def test_kernel_on_a_full_size_frame(vid):
    f = make_frame("random", 1080, 1920, 3, seed=3)
    assert_sdr(vid.blit_probe(f, 1920, 540, 1), VR.blit(f, 1920, 1080, 3, 1920, 540, 1), "1920x1080 -> 1920x540")


def test_scalar_restatement_on_the_device_too(vid):
    """the literal per-sample form, against the kernel directly (small: it is a Python loop)"""
    f = make_frame("random", 6, 7, 3, seed=9)
    assert_sdr(vid.blit_probe(f, 5, 3, 2), VR.blit_scalar(f, 7, 6, 3, 5, 3, 2), "scalar form")


# ------------------------------------------------------------------------------------------------------------- through the context
def expect(frame, fw, fh, ss):
    sdr = VR.blit(frame, frame.shape[1], frame.shape[0], frame.shape[2], fw, fh, ss)
    c16, ansi, rgba = CR.encode(sdr)
    return {"sdr": sdr, "color16": c16, "ansi": ansi, "rgba": rgba}


def assert_outputs(got, want, what):
    for k, a in got.items():
        if k == "sdr":
            assert_sdr(a, want[k], f"{what} sdr")
        else:
            assert a.shape == want[k].shape and np.array_equal(a, want[k]), f"{what} {k}: {np.count_nonzero(a != want[k])} differ"


@pytest.mark.parametrize("fw,fh,ss,sw,sh,bpp", [(37, 11, 2, 64, 48, 3), (80, 45, 1, 33, 50, 4), (1, 1, 1, 20, 10, 3), (21, 9, 3, 8, 8, 4)])
def test_blit_of_a_fresh_context_equals_the_hook_and_the_restatements(product_lib, fw, fh, ss, sw, sh, bpp):
    """no scene: a context that never saw ycge_scene_upload blits; each destination alone and all together"""
    with VideoRenderer(fw, fh, ss, lib=product_lib) as v:
        f = make_frame("random", sh, sw, bpp, seed=fw)
        want = expect(f, fw, fh, ss)
        assert_sdr(v.blit_probe(f, fw, fh, ss), want["sdr"], "hook")
        assert_outputs(v.TryFlipAndBlit(f, color16=True, ansi=True, rgba=True, sdr=True), want, "all")
        for alone in ("sdr", "color16", "ansi", "rgba"):
            got = v.TryFlipAndBlit(f, **{k: k == alone for k in ("sdr", "color16", "ansi", "rgba")})
            assert list(got) == [alone]
            assert_outputs(got, want, f"{alone} alone")
        cw, ch = fw + 3, fh + 2
        for clear, vp, with_sdr in ((True, (0, 0), False), (False, (2, 1), True), (False, (-1, 0), False)):
            r = v.TryFlipAndBlitAnsi(f, cw, ch, viewport=vp, clear_screen=clear, sdr=with_sdr, default_fg=11, default_bg=4)
            stream = r[0] if with_sdr else r
            if with_sdr:
                assert_sdr(r[1], want["sdr"], "ansi form sdr")
            assert stream == A.stream(want["ansi"], cw, ch, vp, 11, 4, clear), (clear, vp)


def test_pageable_and_page_locked_frames_and_destinations(product_lib):
    fw, fh, ss = 40, 12, 2
    with VideoRenderer(fw, fh, ss, lib=product_lib) as v:
        r = v._r
        src = make_frame("random", 30, 50, 3, seed=5)
        want = expect(src, fw, fh, ss)
        cw, ch = 41, 12
        cap = RaytraceRenderer.ansi_stream_bound(cw, ch, v.L)
        for frame_locked in (False, True):
            for dst_locked in (False, True):
                f = src
                if frame_locked:
                    f = r._page_locked_zeros(src.shape, np.uint8)[0]
                    f[...] = src
                    assert v.L.ycge_debug_is_page_locked(f.ctypes.data_as(C.c_void_p), C.c_size_t(f.nbytes)) == 1
                shapes = r.chexel_shapes()
                out = {k: (r._page_locked_zeros(shp, dt)[0] if dst_locked else np.zeros(shp, dt)) for k, (shp, dt) in shapes.items()}
                assert_outputs(v.TryFlipAndBlit(f, out=out), want, f"frame locked {frame_locked}, destinations locked {dst_locked}")
                stream = r._page_locked_zeros((cap + 64,), np.uint8)[0] if dst_locked else np.zeros(cap + 64, np.uint8)
                stream[...] = CANARY
                n = C.c_size_t(0)
                s2 = r._page_locked_zeros(shapes["sdr"][0])[0] if dst_locked else np.zeros(shapes["sdr"][0], np.float32)
                r._check(v.L.ycge_video_blit_ansi(v.ctx, f.ctypes.data_as(U8P), 50, 30, 3, cw, ch, 0, 0, 7, 0, 1, stream.ctypes.data_as(U8P), cap, C.byref(n),
                                                  s2.ctypes.data_as(C.POINTER(C.c_float))))
                assert stream[:n.value].tobytes() == A.stream(want["ansi"], cw, ch, clear=True) and (stream[n.value:] == CANARY).all()      # its exact length, never a byte past it
                assert_sdr(s2, want["sdr"], "stream form sdr")


def test_resize_and_the_table_cache(product_lib):
    with VideoRenderer(30, 10, 1, lib=product_lib) as v:
        f = make_frame("random", 24, 32, 3, seed=1)
        assert_outputs(v.TryFlipAndBlit(f, sdr=True, ansi=True), expect(f, 30, 10, 1), "before")
        for (fw, fh, ss) in ((17, 23, 2), (30, 10, 3), (64, 5, 1)):          # the geometry follows ycge_resize
            v.Resize(fw, fh, ss)
            assert_outputs(v.TryFlipAndBlit(f, sdr=True, color16=True, rgba=True), expect(f, fw, fh, ss), f"resized to {fw}x{fh} ss {ss}")
        # only the source's size changes between calls: the tables are rebuilt for each, and again for the first
        for (sw, sh) in ((32, 24), (24, 32), (33, 24), (32, 24), (32, 25), (32, 24)):
            g = make_frame("random", sh, sw, 3, seed=sw * sh)
            assert_outputs(v.TryFlipAndBlit(g, sdr=True), expect(g, 64, 5, 1), f"source {sw}x{sh}")
        # ... and the hook's geometry leaves the context's alone
        v.blit_probe(f, 9, 9, 2)
        assert_outputs(v.TryFlipAndBlit(f, sdr=True), expect(f, 64, 5, 1), "after the hook")


# ------------------------------------------------------------------------------------------------------------- frame state
STATE_BUFFERS = (abi.BUF_CURRENT_HDR, abi.BUF_G_ALBEDO, abi.BUF_G_NORMAL, abi.BUF_G_DEPTH, abi.BUF_SKY_MASK, abi.BUF_TAA_HISTORY, abi.BUF_PREV_NORMAL,
                 abi.BUF_PREV_DEPTH, abi.BUF_PREV_SKY, abi.BUF_DENOISED)
DEBUG_BUFFERS = (abi.BUF_RAYS, abi.BUF_PRIM_ID, abi.BUF_SUB_ID, abi.BUF_HIT_T, abi.BUF_RNG_STATE)


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_a_blit_between_frames_changes_nothing_a_frame_reads(product_lib):
    """config 1: frame / frame / blit / frame gives the third frame of three frames with no blit - in every ycge_read_buffer buffer (TAA
    history included), the SDR, the exposure and the statistics' frame number"""
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    a = RaytraceRenderer(flat, w, h, pose["fov"], ss, capture_debug=True, lib=product_lib)
    b = RaytraceRenderer(flat, w, h, pose["fov"], ss, capture_debug=True, lib=product_lib)
    try:
        v = VideoRenderer(renderer=b)
        f = make_frame("random", 48, 64, 3, seed=2)
        want = expect(f, w, h, ss)
        for g in (a, b):
            g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        for k in range(3):
            if k == 2:
                assert_outputs(v.TryFlipAndBlit(f, sdr=True, color16=True, ansi=True, rgba=True), want, "blit between frames")
                assert v.TryFlipAndBlitAnsi(f, w + 1, h) == A.stream(want["ansi"], w + 1, h)
            sa, sb = a.TryFlipAndBlit(want_sdr=True), b.TryFlipAndBlit(want_sdr=True)
            assert pu.bits_equal(sa, sb), k
            assert a.stats.frame == b.stats.frame and a.stats.history_reset == b.stats.history_reset and a.stats.exposure == b.stats.exposure, k
        for which in STATE_BUFFERS + DEBUG_BUFFERS:
            assert same_bytes(a.read(which), b.read(which)), which
        # and a fourth frame still agrees (the exposure state and the history went on from the same values)
        assert pu.bits_equal(a.TryFlipAndBlit(want_sdr=True), b.TryFlipAndBlit(want_sdr=True))
    finally:
        a.close(); b.close()


def test_a_blit_between_frames_in_flight_joins_them_and_changes_nothing(product_lib):
    sc, w, h, ss, pose = scenes.config_scene(1)
    flat = flatten(sc)
    a = RaytraceRenderer(flat, w, h, pose["fov"], ss, lib=product_lib)
    b = RaytraceRenderer(flat, w, h, pose["fov"], ss, lib=product_lib)
    try:
        v = VideoRenderer(renderer=b)
        f = make_frame("checker", 20, 30, 4, seed=2)
        want = expect(f, w, h, ss)
        for g in (a, b):
            g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        a.RenderAsync(); a.RenderAsync(); a.Wait()
        b.RenderAsync()
        assert b.flight_info()["frames_outstanding"] == 1
        assert_outputs(v.TryFlipAndBlit(f, sdr=True, ansi=True), want, "blit between frames in flight")
        assert b.flight_info()["frames_outstanding"] == 0          # joined, like every entry point except the scene queries
        b.RenderAsync(); b.Wait()
        for which in STATE_BUFFERS[:-1]:          # (no post stage ran: nothing denoised)
            assert same_bytes(a.read(which), b.read(which)), which
        assert pu.bits_equal(a.TryFlipAndBlit(want_sdr=True), b.TryFlipAndBlit(want_sdr=True))
        assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- refusals
def _blit(v, ctx, frame, w, h, bpp, out):
    p = frame.ctypes.data_as(U8P) if frame is not None else None
    return v.L.ycge_video_blit(ctx, p, w, h, bpp, *RaytraceRenderer._chexel_pointers(out))


def _blit_ansi(v, ctx, frame, w, h, bpp, cw, ch, stream, cap, n, fg=7, bg=0, sdr=None):
    return v.L.ycge_video_blit_ansi(ctx, frame.ctypes.data_as(U8P) if frame is not None else None, w, h, bpp, cw, ch, 0, 0, fg, bg, 0,
                                    stream.ctypes.data_as(U8P) if stream is not None else None, cap, C.byref(n) if n is not None else None,
                                    sdr.ctypes.data_as(C.POINTER(C.c_float)) if sdr is not None else None)


def test_refusals_leave_the_context_usable_and_the_arrays_alone(product_lib):
    fw, fh = 20, 6
    with VideoRenderer(fw, fh, 1, lib=product_lib) as v:
        r = v._r
        f = make_frame("random", 10, 12, 3, seed=8)
        want = expect(f, fw, fh, 1)
        out = {k: np.full(shp, CANARY if dt == np.uint8 else 7.0, dt) for k, (shp, dt) in r.chexel_shapes().items()}
        cw, ch = fw, fh
        cap = RaytraceRenderer.ansi_stream_bound(cw, ch, v.L)
        stream = np.full(cap, CANARY, np.uint8)
        n = C.c_size_t(12345)

        def untouched():
            assert all((a == (CANARY if a.dtype == np.uint8 else 7.0)).all() for a in out.values()) and (stream == CANARY).all() and n.value == 12345

        bad = [(None, 12, 10, 3), (f, 0, 10, 3), (f, 12, 0, 3), (f, -1, 10, 3), (f, 12, 10, 2), (f, 12, 10, 5), (f, 12, 10, 0), (f, 1 << 15, 1 << 15, 3), (f, 1 << 16, 1 << 13, 4)]
        for (fr, w, h, bpp) in bad:
            assert _blit(v, v.ctx, fr, w, h, bpp, out) == abi.YCGE_ERR_INVALID_ARG, (w, h, bpp)
            assert v.L.ycge_last_error(v.ctx)
            assert _blit_ansi(v, v.ctx, fr, w, h, bpp, cw, ch, stream, cap, n, sdr=out["sdr"]) == abi.YCGE_ERR_INVALID_ARG, (w, h, bpp)
            untouched()
        assert _blit(v, v.ctx, f, 12, 10, 3, {}) == abi.YCGE_ERR_INVALID_ARG          # all destinations NULL
        assert _blit(v, None, f, 12, 10, 3, out) == abi.YCGE_ERR_INVALID_ARG
        # what ycge_render_frame_ansi refuses that does not concern a frame's post stage
        for kw in (dict(stream=None), dict(n=None), dict(cw=0), dict(ch=-3), dict(fg=16), dict(bg=-1), dict(cap=cap - 1), dict(cw=1 << 15, ch=1 << 15, cap=1 << 40)):
            args = dict(cw=cw, ch=ch, stream=stream, cap=cap, n=n, fg=7, bg=0)
            args.update(kw)
            assert _blit_ansi(v, v.ctx, f, 12, 10, 3, args["cw"], args["ch"], args["stream"], args["cap"], args["n"], args["fg"], args["bg"], sdr=out["sdr"]) == abi.YCGE_ERR_INVALID_ARG, kw
            untouched()
        # the context blits on
        assert_outputs(v.TryFlipAndBlit(f, sdr=True, color16=True, ansi=True, rgba=True), want, "after the refusals")
        assert v.TryFlipAndBlitAnsi(f, cw, ch) == A.stream(want["ansi"], cw, ch)
        untouched()


def test_a_peer_context_refuses_and_its_root_blits(product_lib):
    sc, w, h, ss, pose = scenes.config_scene(1)
    r = RaytraceRenderer(flatten(sc), w, h, pose["fov"], ss, devices=[0, 0], lib=product_lib)
    try:
        v = VideoRenderer(renderer=r)
        peer = C.c_void_p(r.L.ycge_debug_peer_context(r.ctx, 0))
        assert peer.value
        f = make_frame("random", 9, 16, 3, seed=4)
        out = {k: np.full(shp, CANARY if dt == np.uint8 else 7.0, dt) for k, (shp, dt) in r.chexel_shapes().items()}
        assert _blit(v, peer, f, 16, 9, 3, out) == abi.YCGE_ERR_INVALID_ARG
        cap = RaytraceRenderer.ansi_stream_bound(w, h, r.L)
        stream, n = np.full(cap, CANARY, np.uint8), C.c_size_t(5)
        assert _blit_ansi(v, peer, f, 16, 9, 3, w, h, stream, cap, n) == abi.YCGE_ERR_INVALID_ARG
        assert all((a == (CANARY if a.dtype == np.uint8 else 7.0)).all() for a in out.values()) and (stream == CANARY).all() and n.value == 5
        r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        before = r.TryFlipAndBlit(want_sdr=True)
        assert_outputs(v.TryFlipAndBlit(f, sdr=True, color16=True, ansi=True, rgba=True), expect(f, w, h, ss), "root of a two-context peer push")
        assert np.isfinite(before).all() and np.isfinite(r.TryFlipAndBlit(want_sdr=True)).all()
    finally:
        r.close()


def test_allocation_failure_in_the_first_blit(product_lib):
    """lib/var_faultinject.so: the n-th host allocation of a context's first blit fails -> YCGE_ERR_OUT_OF_MEMORY; the arrays of a failed call
    are never written afterwards, and the retry is clean"""
    L = abi.load_library(build.build_variant("faultinject"))
    L.ycge_debug_fail_allocation.restype = C.c_int
    L.ycge_debug_fail_allocation.argtypes = [C.c_int64]
    fw, fh, ss = 24, 7, 2
    f = make_frame("random", 18, 26, 3, seed=6)
    want = expect(f, fw, fh, ss)
    failed, n = 0, 0
    while True:
        v = VideoRenderer(fw, fh, ss, lib=L)
        try:
            arrs = {k: np.zeros(shp, dt) for k, (shp, dt) in v._r.chexel_shapes().items()}
            L.ycge_debug_fail_allocation(n)
            rc = _blit(v, v.ctx, f, 26, 18, 3, arrs)
            left = L.ycge_debug_fail_allocation(-1)
            assert rc in (abi.YCGE_OK, abi.YCGE_ERR_OUT_OF_MEMORY), (n, rc, L.ycge_last_error(v.ctx))
            if rc == abi.YCGE_ERR_OUT_OF_MEMORY:
                failed += 1
                assert b"bad_alloc" in L.ycge_last_error(v.ctx)
                for arr in arrs.values():
                    arr[...] = 0          # (what the failed call may have written before it failed is not the question)
                for k in range(2):
                    assert_outputs(v.TryFlipAndBlit(f, sdr=True, color16=True, ansi=True, rgba=True), want, f"n = {n}, retry {k}")
                assert not any(arr.any() for arr in arrs.values()), n
            else:
                assert_outputs(arrs, want, f"n = {n}")
                if left >= 0:
                    break
        finally:
            v.close()
        n += 1 if n < 40 else max(1, n // 3)
    assert failed >= 1
