"""The delta ANSI stream on the GPU: the delta kernels through their hook (ycge_test_ansi_delta) on pairs a frame never produces, the
frames of ycge_render_frame_ansi_delta against the restatement (tests/ansi_delta_restatement.py) of the SDR arrays the calls returned and
against a terminal model fed every stream in order, and the state rules one by one.  Every stream is compared byte for byte, with its
exact length and a canary behind it, and every out_info with the restatement's."""
import ctypes as C

import numpy as np
import pytest

import ansi_delta_restatement as D
import ansi_stream_restatement as A
import parity_util as pu
import test_gpu_ansi_stream as S
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VideoRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
U8P = C.POINTER(C.c_uint8)
CANARY = S.CANARY


def hook(g, prev, cur, cw, ch, viewport=(0, 0), fg=7, bg=0, clear=False, gap=1):
    """ycge_test_ansi_delta on (fbH, fbW, 2) pairs (prev None: the keyframe) -> (stream, info); nothing past the length was written"""
    cur = np.ascontiguousarray(cur, dtype=np.uint8)
    prev = None if prev is None else np.ascontiguousarray(prev, dtype=np.uint8)
    fbH, fbW = cur.shape[:2]
    cap = RaytraceRenderer.ansi_stream_bound(cw, ch, g.L)
    out = np.full(cap + 64, CANARY, np.uint8)
    n, info = C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    fn = g.L.ycge_test_ansi_delta
    fn.restype, fn.argtypes = abi.ANSI_DELTA_HOOK_PROTOTYPES["ycge_test_ansi_delta"]
    g._check(fn(g.ctx, prev.ctypes.data_as(U8P) if prev is not None else None, cur.ctypes.data_as(U8P), fbW, fbH, cw, ch, viewport[0], viewport[1], fg, bg,
                int(clear), gap, out.ctypes.data_as(U8P), cap, C.byref(n), info))
    assert n.value <= cap
    assert (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), dict(zip(D.INFO, (int(v) for v in info)))


def check(g, prev, cur, cw, ch, viewport=(0, 0), fg=7, bg=0, gap=1, what=""):
    got, info = hook(g, prev, cur, cw, ch, viewport, fg, bg, False, gap)
    want, winfo = D.delta(prev, cur, cw, ch, viewport, fg, bg, gap)
    S.assert_stream(got, want, what)
    assert info == winfo, (what, info, winfo)
    return got, info


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


def _frames(rng, h, w, density):
    """prev with long runs of equal cells and three-digit indices; cur = prev with `density` of its cells redrawn"""
    prev = (rng.integers(0, 3, (h, w, 2)) * 100 + 5).astype(np.uint8)
    redraw = rng.random((h, w, 1)) < density
    cur = np.where(redraw, rng.integers(0, 256, (h, w, 2)), prev).astype(np.uint8)
    return prev, cur


# ------------------------------------------------------------------------------------------------------------- 1: the kernels alone
@pytest.mark.parametrize("gap", [0, 1, 8])
@pytest.mark.parametrize("w,h", [(7, 3), (1100, 3), (33, 70)])
def test_hook_densities(enc, w, h, gap):
    rng = np.random.default_rng(w * 1000 + h * 10 + gap)
    for density in (0.0, 1 / 256, 0.5, 1.0):
        prev, cur = _frames(rng, h, w, density)
        _, info = check(enc, prev, cur, w, h, gap=gap, what=(w, h, gap, density))
        assert info["keyframe"] == 0 and info["changed"] == int((prev != cur).any(axis=-1).sum())


@pytest.mark.parametrize("w,h", [(1100, 3), (33, 70), (512, 5)], ids=["1100x3", "33x70", "512x5-row-end-on-a-tile-boundary"])
def test_hook_runs_and_gap_windows_across_the_tile_and_lane_boundaries(enc, w, h):
    rng = np.random.default_rng(w + h)
    prev, _ = _frames(rng, h, w, 0.0)
    groups = [(1023, 1024), (1021, 1022, 1023, 1024, 1025, 1026), (1022, 1025), (1023, 1025), (1020, 1024, 1028), (1015, 1024), (1016, 1025), (1014, 1024),
              (1019, 1020, 1029), (1023,), (1024,), (2047, 2048), (2044, 2051)]
    for cells in groups:
        cells = [c for c in cells if c < w * h]
        cur = prev.copy()
        for c in cells:
            cur[c // w, c % w] = (cur[c // w, c % w] + (1, 101)).astype(np.uint8)
        for gap in (0, 1, 2, 8):
            check(enc, prev, cur, w, h, gap=gap, what=(w, h, cells, gap))
    if w == 512:          # (511, 1) and (0, 2) are cells 1023 and 1024: two runs whatever the gap
        cur = prev.copy()
        cur[1, 511], cur[2, 0] = (250, 251), (252, 253)
        got, info = check(enc, prev, cur, w, h, gap=8)
        assert info == dict(keyframe=0, changed=2, emitted=3, runs=3) and b"\x1b[2;512H" in got and b"\x1b[3;1H" in got


def test_hook_four_digit_rows_and_columns(enc):
    rng = np.random.default_rng(1001)
    # (w, h, the cells (y, x) that change while their left neighbours rest, the cursor moves they must start)
    for w, h, cells, tokens in [(3, 1001, [(1000, 0), (999, 0)], [b"\x1b[1001;1H", b"\x1b[1000;1H"]),
                                (1001, 3, [(1, 1000), (0, 999)], [b"\x1b[2;1001H", b"\x1b[1;1000H"])]:
        prev, cur = _frames(rng, h, w, 0.5)
        for y, x in cells:
            cur[y, x], prev[y, x] = (1, 2), (3, 4)
            if x > 0:
                prev[y, x - 1] = cur[y, x - 1]
        got, _ = check(enc, prev, cur, w, h, gap=0, what=(w, h))
        assert all(t in got for t in tokens), (w, h)


@pytest.mark.parametrize("cw,ch,vp", [(31, 17, (0, 0)), (31, 17, (5, 3)), (31, 17, (-4, -2)), (31, 17, (-20, 2)), (31, 17, (40, 0)),
                                      (31, 17, (0, 30)), (31, 17, (-100, -100)), (12, 10, (0, 0)), (1, 1, (0, 0)), (1, 1, (1, 0)),
                                      (1, 1, (-19, -9)), (21, 11, (0, 0))])
def test_hook_geometry(enc, cw, ch, vp):
    rng = np.random.default_rng(abs(cw * 100 + ch + 7 * vp[0] + vp[1]))
    prev, cur = _frames(rng, 11, 20, 0.3)
    for gap in (0, 1, 8):
        check(enc, prev, cur, cw, ch, vp, 2, 14, gap, what=(cw, ch, vp, gap))


def test_hook_one_by_one_framebuffer(enc):
    prev, cur = np.array([[[255, 0]]], np.uint8), np.array([[[255, 1]]], np.uint8)
    for cw, ch, vp in [(1, 1, (0, 0)), (3, 2, (1, 1)), (3, 2, (2, 1)), (3, 2, (5, 5))]:
        check(enc, prev, cur, cw, ch, vp, what=(cw, ch, vp))
        check(enc, cur, cur, cw, ch, vp, what=(cw, ch, vp, "still"))


def test_hook_without_prev_is_the_full_stream(enc):
    rng = np.random.default_rng(77)
    _, p = _frames(rng, 11, 20, 1.0)
    for cw, ch, vp, clear in [(21, 11, (0, 0), False), (31, 17, (5, 3), True), (1100, 3, (0, 0), False)]:
        got, info = hook(enc, None, p, cw, ch, vp, 2, 14, clear, gap=3)
        S.assert_stream(got, A.stream(p, cw, ch, vp, 2, 14, clear), (cw, ch, vp, clear))
        S.assert_stream(got, S.hook(enc, p, cw, ch, vp, 2, 14, clear), "the full stream's hook")
        assert info == dict(keyframe=1, changed=0, emitted=0, runs=0)
    got, info = hook(enc, p, p, 21, 11, clear=True)          # clear_screen: a keyframe whatever prev is
    S.assert_stream(got, A.stream(p, 21, 11, clear=True), "clear")
    assert info["keyframe"] == 1


def test_hook_random_pairs_641x181(enc):
    rng = np.random.default_rng(181)
    prev, cur = _frames(rng, 180, 640, 1 / 8)
    _, info = check(enc, prev, cur, 641, 181, gap=1, what="640x180 in 641x181")
    assert info["runs"] > 1000 and info["emitted"] > info["changed"]


# ------------------------------------------------------------------------------------------------------------- 2: frames
FRAME_CASES = [c for c in S.FRAME_CASES if c[0] in (1, 2, 5)]


@pytest.mark.parametrize("n,w,h,ss", FRAME_CASES, ids=[f"c{c[0]}-{c[1]}x{c[2]}-ss{c[3]}" for c in FRAME_CASES])
def test_frames_equal_the_plain_frame_the_restatement_and_the_terminal(product_lib, n, w, h, ss):
    a, b, pose = S.twins(n, w, h, ss)
    try:
        cw, ch, gap = w + 1, h, 1                                  # the product's console: one column wider than the framebuffer
        screen, last = D.Screen(cw, ch), None
        for k, cam in enumerate([0, 0, 0, 1, 1, 1]):               # at rest for three frames, moved, at rest again
            S.move((a, b), pose, cam)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, info, s2 = b.TryFlipAndBlitAnsiDelta(cw, ch, merge_gap=gap, sdr=True)
            assert pu.bits_equal(sdr, s2), (n, k)
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
            full = A.frame_stream(s2, cw, ch)
            if k == 0:
                S.assert_stream(stream, full, f"config {n}: the first stream is a keyframe")
                assert info == dict(keyframe=1, changed=0, emitted=0, runs=0)
            else:
                want, winfo = D.frame_delta(last, s2, cw, ch, gap=gap)
                S.assert_stream(stream, want, f"config {n} frame {k}")
                assert info == winfo, (n, k, info, winfo)
                assert len(stream) <= len(full)
            assert screen.feed(stream).state() == D.Screen(cw, ch).feed(full).state(), (n, k)
            last = s2
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 3: the state rules
CW, CH = 81, 45


@pytest.fixture()
def one(product_lib):
    sc, _, _, _, pose = scenes.config_scene(1, t01=0.5)
    g = RaytraceRenderer(flatten(sc), 80, 45, pose.get("fov", 45.0), 1)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    yield g, pose
    g.close()


def step(g, last, cw=CW, ch=CH, keyframe_expected=False, what="", **kw):
    """one delta frame of g, held to the restatement against `last` (the SDR of the stream before) or to the keyframe; -> its SDR"""
    kw.setdefault("merge_gap", 1)
    stream, info, s = g.TryFlipAndBlitAnsiDelta(cw, ch, sdr=True, **kw)
    want, winfo = D.frame_delta(None if keyframe_expected else last, s, cw, ch, kw.get("viewport", (0, 0)), kw.get("default_fg", 7), kw.get("default_bg", 0),
                                kw["merge_gap"], kw.get("clear_screen", False))
    S.assert_stream(stream, want, what)
    assert info == winfo and info["keyframe"] == int(keyframe_expected), (what, info, winfo)
    return s


def test_resize_makes_the_next_call_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True, what="first")
    s = step(g, s, what="delta")
    g.Resize(96, 30, 1)
    s = step(g, s, 97, 30, keyframe_expected=True, what="after Resize")
    s = step(g, s, 97, 30, what="delta at the new size")
    g.Resize(96, 30, 1)                                            # (to the same size: the history is gone all the same)
    step(g, s, 97, 30, keyframe_expected=True, what="after Resize to the same size")


def test_a_changed_viewport_or_default_makes_the_next_call_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    s = step(g, s, viewport=(1, 0), keyframe_expected=True, what="viewport")
    s = step(g, s, viewport=(1, 0), what="delta at the new viewport")
    s = step(g, s, viewport=(1, 0), default_bg=4, keyframe_expected=True, what="default colour")
    s = step(g, s, CW + 1, CH, viewport=(1, 0), default_bg=4, keyframe_expected=True, what="console")
    step(g, s, CW + 1, CH, viewport=(1, 0), default_bg=4, merge_gap=5, what="another merge_gap is no other geometry")


def test_keyframe_and_clear_screen_give_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s, keyframe=True, keyframe_expected=True, what="keyframe = 1")
    s = step(g, s, what="delta")
    stream, info = g.TryFlipAndBlitAnsiDelta(CW, CH, clear_screen=True, merge_gap=1)
    assert info["keyframe"] == 1 and stream.startswith(b"\x1b[2J\x1b[H\x1b[1;1H")
    s = step(g, s, clear_screen=True, keyframe_expected=True, what="clear_screen")
    step(g, s, what="delta again")


def test_an_interleaved_full_stream_makes_the_next_call_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    g.TryFlipAndBlit()                                             # (a plain frame shows the terminal nothing)
    S.move([g], pose, 1)
    s = step(g, s, what="a delta against the last stream, two frames back")
    g.TryFlipAndBlitAnsi(CW, CH)
    s = step(g, s, keyframe_expected=True, what="after TryFlipAndBlitAnsi")
    step(g, s, what="delta")


def _call(g, cw, ch, out, cap, n, info=None, sdr=None, gap=1, keyframe=0, clear=0):
    return g.L.ycge_render_frame_ansi_delta(g.ctx, cw, ch, 0, 0, 7, 0, clear, gap, keyframe, out.ctypes.data_as(U8P), cap, C.byref(n), info,
                                            sdr.ctypes.data_as(C.POINTER(C.c_float)) if sdr is not None else None, None)


def test_a_refused_call_leaves_prev_alone(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    frame = g.stats.frame
    cap = RaytraceRenderer.ansi_stream_bound(CW, CH, g.L)
    out, n, info = np.zeros(cap, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)()
    for kw, words in [(dict(gap=9), [b"merge_gap 9"]), (dict(gap=-1), [b"merge_gap -1"]), (dict(cap=cap - 1), [b"capacity %d" % (cap - 1), b"bound %d" % cap])]:
        rc = _call(g, CW, CH, out, kw.get("cap", cap), n, info, gap=kw.get("gap", 1))
        msg = g.L.ycge_last_error(g.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), (kw, rc, msg)
    assert not out.any() and n.value == 0 and list(info) == [0, 0, 0, 0]
    S.move([g], pose, 2)
    step(g, s, what="the next delta is against the frame before the refusals")
    assert g.stats.frame == frame + 1


def test_a_video_delta_follows_a_ray_traced_one_on_the_shared_context(one):
    g, pose = one
    v = VideoRenderer(renderer=g)
    rng = np.random.default_rng(3)
    movie = rng.integers(0, 256, (36, 64, 3)).astype(np.uint8)
    s = step(g, None, keyframe_expected=True)
    stream, info, vs = v.TryFlipAndBlitAnsiDelta(movie, CW, CH, merge_gap=2, sdr=True)
    want, winfo = D.frame_delta(s, vs, CW, CH, gap=2)
    S.assert_stream(stream, want, "video against the ray-traced frame")
    assert info == winfo and info["keyframe"] == 0 and info["changed"] > 0
    stream, info = v.TryFlipAndBlitAnsiDelta(movie, CW, CH, merge_gap=2)
    assert (stream, info) == D.frame_delta(vs, vs, CW, CH, gap=2)         # the same picture: the last cell alone
    assert info == dict(keyframe=0, changed=0, emitted=1, runs=1)
    s = step(g, vs, what="ray-traced against the video frame")
    v.TryFlipAndBlitAnsi(movie, CW, CH)
    step(g, s, keyframe_expected=True, what="after the video's full stream")


def test_pageable_and_page_locked_destinations(one):
    g, pose = one
    cap = RaytraceRenderer.ansi_stream_bound(CW, CH, g.L)
    last = None
    for k, form in enumerate(["pageable", "locked", "pageable", "locked"]):
        S.move([g], pose, k)
        if form == "locked":
            out = g._page_locked_zeros((cap + 64,), np.uint8)[0]
            s2 = g._page_locked_zeros((45, 80, 2, 3))[0]
        else:
            out, s2 = np.zeros(cap + 64, np.uint8), np.zeros((45, 80, 2, 3), np.float32)
        out[...] = CANARY
        n, info = C.c_size_t(0), (C.c_uint32 * 4)()
        g._check(_call(g, CW, CH, out, cap, n, info, s2))
        assert (out[n.value:] == CANARY).all(), k
        want, winfo = D.frame_delta(last, s2, CW, CH)
        S.assert_stream(out[:n.value].tobytes(), want, f"{form} {k}")
        assert dict(zip(D.INFO, info)) == winfo
        last = s2.copy()


def test_peer_push_contexts_on_one_gpu(product_lib):
    a, b, pose = S.twins(2, 160, 45, 1, devices=[0, 0, 0])
    try:
        last = None
        for k in range(3):
            S.move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, info, s2 = b.TryFlipAndBlitAnsiDelta(161, 45, merge_gap=0, sdr=True)
            assert pu.bits_equal(sdr, s2), k
            want, winfo = D.frame_delta(last, s2, 161, 45, gap=0)
            S.assert_stream(stream, want, f"peer push {k}")
            assert info == winfo
            last = s2
    finally:
        a.close(); b.close()


def test_the_lean_slab_refusal_is_that_of_the_full_stream(product_lib):
    cfg = abi.default_config()
    cfg.multi_device_exchange = abi.EXCHANGE_RCCL
    sc, w, h, ss, pose = scenes.config_scene(1)
    lean = RaytraceRenderer(flatten(sc), 80, 45, pose["fov"], 1, cfg=cfg, devices=[0], slab_albedo=False)
    try:
        cap = RaytraceRenderer.ansi_stream_bound(CW, CH, lean.L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        rc = _call(lean, CW, CH, out, cap, n)
        delta_msg = lean.L.ycge_last_error(lean.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and b"lean slabs" in delta_msg
        assert S._call(lean, CW, CH, out, cap, n) == abi.YCGE_ERR_INVALID_ARG and lean.L.ycge_last_error(lean.ctx) == delta_msg
        assert not out.any() and n.value == 0
    finally:
        lean.close()
