"""The 24-bit colour ANSI streams on the GPU: the stream kernels through their hooks (ycge_test_ansi_rgb_stream, ycge_test_ansi_rgb_delta)
on colour images a frame never produces, the frames of ycge_render_frame_ansi_rgb / _rgb_delta against the restatement
(tests/ansi_rgb_restatement.py) of the SDR arrays the calls returned and against a terminal model fed every stream in order, and the state
rules one by one.  Every stream is compared byte for byte, with its exact length and a canary behind it; every out_info and every
out_shown with the restatement's."""
import ctypes as C

import numpy as np
import pytest

import ansi_delta_restatement as D
import ansi_rgb_restatement as R
import ansi_stream_restatement as A
import parity_util as pu
import test_gpu_ansi_stream as S
from yetanotherconsolegameengine_amd import abi, scenes
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VideoRenderer
from yetanotherconsolegameengine_amd.scene import flatten

pytestmark = pytest.mark.gpu
U8P = C.POINTER(C.c_uint8)
CANARY = S.CANARY
DIGIT_EDGES = np.array([0, 9, 10, 99, 100, 255], np.uint8)


def hook_stream(g, rgba, cw, ch, viewport=(0, 0), fg=7, bg=0, clear=False):
    """ycge_test_ansi_rgb_stream on a (2 fbH, fbW, 4) plane -> the stream; nothing past its length was written"""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    fbH, fbW = rgba.shape[0] // 2, rgba.shape[1]
    cap = RaytraceRenderer.ansi_rgb_stream_bound(cw, ch, g.L)
    out = np.full(cap + 64, CANARY, np.uint8)
    n = C.c_size_t(0)
    fn = g.L.ycge_test_ansi_rgb_stream
    fn.restype, fn.argtypes = abi.ANSI_RGB_HOOK_PROTOTYPES["ycge_test_ansi_rgb_stream"]
    g._check(fn(g.ctx, rgba.ctypes.data_as(U8P), fbW, fbH, cw, ch, viewport[0], viewport[1], fg, bg, int(clear), out.ctypes.data_as(U8P), cap, C.byref(n)))
    assert n.value <= cap and (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes()


def hook_delta(g, shown, cur, cw, ch, viewport=(0, 0), fg=7, bg=0, clear=False, gap=3, tol=0):
    """ycge_test_ansi_rgb_delta (shown None: the keyframe) -> (stream, info, out_shown); nothing past the length was written"""
    cur = np.ascontiguousarray(cur, dtype=np.uint8)
    shown = None if shown is None else np.ascontiguousarray(shown, dtype=np.uint8)
    fbH, fbW = cur.shape[0] // 2, cur.shape[1]
    cap = RaytraceRenderer.ansi_rgb_stream_bound(cw, ch, g.L)
    out = np.full(cap + 64, CANARY, np.uint8)
    new = np.full(cur.shape, 0x5A, np.uint8)
    n, info = C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    fn = g.L.ycge_test_ansi_rgb_delta
    fn.restype, fn.argtypes = abi.ANSI_RGB_HOOK_PROTOTYPES["ycge_test_ansi_rgb_delta"]
    g._check(fn(g.ctx, shown.ctypes.data_as(U8P) if shown is not None else None, cur.ctypes.data_as(U8P), fbW, fbH, cw, ch, viewport[0], viewport[1], fg, bg,
                int(clear), gap, tol, out.ctypes.data_as(U8P), cap, C.byref(n), info, new.ctypes.data_as(U8P)))
    assert n.value <= cap and (out[n.value:] == CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), dict(zip(R.INFO, (int(v) for v in info))), new


def check_stream(g, rgba, cw, ch, viewport=(0, 0), fg=7, bg=0, clear=False, what=""):
    got = hook_stream(g, rgba, cw, ch, viewport, fg, bg, clear)
    S.assert_stream(got, R.stream(rgba, cw, ch, viewport, fg, bg, clear), what)
    return got


def check(g, shown, cur, cw, ch, viewport=(0, 0), fg=7, bg=0, gap=3, tol=0, what=""):
    got, info, new = hook_delta(g, shown, cur, cw, ch, viewport, fg, bg, False, gap, tol)
    want, winfo, wnew = R.delta(shown, cur, cw, ch, viewport, fg, bg, gap, tol)
    S.assert_stream(got, want, what)
    assert info == winfo, (what, info, winfo)
    assert (new == wnew).all(), (what, "out_shown", np.argwhere((new != wnew).any(axis=-1))[:4])
    return got, info, new


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


def _image(rng, h, w):
    """a plane with runs of five equal columns whose channels sit on the digit boundaries, and a random fourth byte"""
    cols = DIGIT_EDGES[rng.integers(0, 6, (2 * h, (w + 4) // 5, 3))]
    p = np.empty((2 * h, w, 4), np.uint8)
    p[..., :3] = np.repeat(cols, 5, axis=1)[:, :w]
    p[..., 3] = rng.integers(0, 256, (2 * h, w))
    return p


def _frames(rng, h, w, density):
    """shown = _image; cur = shown with `density` of its cells redrawn and a third of the others moved by -3..3 in one half-cell"""
    shown = _image(rng, h, w)
    cur = shown.copy()
    if density > 0:
        jitter = rng.integers(-3, 4, (2 * h, w, 3)) * (rng.random((2 * h, w, 1)) < 1 / 3)
        cur[..., :3] = np.clip(cur[..., :3].astype(np.int64) + jitter, 0, 255)
        redraw = np.repeat(rng.random((h, w)) < density, 2, axis=0)[..., None]
        cur[..., :3] = np.where(redraw, rng.integers(0, 256, (2 * h, w, 3)), cur[..., :3])
    return shown, cur


# ------------------------------------------------------------------------------------------------------------- 1: the kernels alone
@pytest.mark.parametrize("w,h", [(7, 3), (1100, 3), (512, 5), (33, 70), (3, 1001), (1001, 3)])
def test_hook_full_stream_shapes(enc, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    got = check_stream(enc, _image(rng, h, w), w, h, what=(w, h, "runs"))
    check_stream(enc, rng.integers(0, 256, (2 * h, w, 4)).astype(np.uint8), w, h, clear=True, what=(w, h, "random"))
    assert b"\x1b[%d;1H" % h in got
    flat = np.zeros((2 * h, w, 4), np.uint8); flat[..., :3] = (100, 9, 255)          # one long run: one escape in all
    got = check_stream(enc, flat, w, h, what=(w, h, "one colour"))
    assert got.count(b"\x1b[38;2;") == 1 and got.count(b"\x1b[48;2;") == 0


def test_hook_channel_digits(enc):
    p = np.zeros((2 * 6, 36, 4), np.uint8)
    for y in range(12):
        for x in range(36):
            p[y, x, :3] = DIGIT_EDGES[[(x + y) % 6, (x // 6 + y) % 6, (x * 5 + y // 2) % 6]]
    got = check_stream(enc, p, 36, 6, what="digit edges")
    assert len(got) < R.bound(36, 6)
    p[..., :3] = 255
    p[::2, ::2, 0] = 254
    p[1::2, 1::2, 2] = 254          # neighbours differ in fg and in bg: every escape at its longest
    assert len(check_stream(enc, p, 36, 6, clear=True, what="longest")) == R.bound(36, 6)


@pytest.mark.parametrize("cw,ch,vp", [(31, 17, (0, 0)), (31, 17, (5, 3)), (31, 17, (-4, -2)), (31, 17, (-20, 2)), (31, 17, (40, 0)),
                                      (31, 17, (0, 30)), (31, 17, (-100, -100)), (12, 10, (0, 0)), (12, 10, (-9, -2)), (1, 1, (0, 0)), (1, 1, (1, 0)),
                                      (1, 1, (-19, -10)), (21, 11, (0, 0))])
def test_hook_geometry(enc, cw, ch, vp):
    rng = np.random.default_rng(abs(cw * 100 + ch + 7 * vp[0] + vp[1]))
    shown, cur = _frames(rng, 11, 20, 0.3)
    check_stream(enc, cur, cw, ch, vp, 2, 14, what=(cw, ch, vp))
    check_stream(enc, cur, cw, ch, vp, 15, 15, True, what=(cw, ch, vp, "clear"))
    for gap, tol in [(0, 0), (1, 1), (8, 3), (3, 255)]:
        check(enc, shown, cur, cw, ch, vp, 2, 14, gap, tol, what=(cw, ch, vp, gap, tol))


def test_hook_one_by_one_framebuffer(enc):
    shown, cur = np.array([[[255, 0, 9, 1]], [[10, 99, 100, 2]]], np.uint8), np.array([[[255, 0, 9, 3]], [[10, 99, 101, 4]]], np.uint8)
    for cw, ch, vp in [(1, 1, (0, 0)), (3, 2, (1, 1)), (3, 2, (2, 1)), (3, 2, (5, 5))]:
        check_stream(enc, cur, cw, ch, vp, what=(cw, ch, vp))
        for tol in (0, 1):
            check(enc, shown, cur, cw, ch, vp, tol=tol, what=(cw, ch, vp, tol))
        check(enc, cur, cur, cw, ch, vp, what=(cw, ch, vp, "still"))
    assert check(enc, shown, cur, 1, 1, tol=0)[1]["changed"] == 1 and check(enc, shown, cur, 1, 1, tol=1)[1]["changed"] == 0


@pytest.mark.parametrize("gap", [0, 1, 8])
@pytest.mark.parametrize("w,h", [(7, 3), (1100, 3), (33, 70)])
def test_hook_densities_and_tolerances(enc, w, h, gap):
    rng = np.random.default_rng(w * 1000 + h * 10 + gap)
    for density in (0.0, 1 / 256, 0.5, 1.0):
        shown, cur = _frames(rng, h, w, density)
        seen = []
        for tol in (0, 1, 3, 255):
            _, info, _ = check(enc, shown, cur, w, h, gap=gap, tol=tol, what=(w, h, gap, density, tol))
            assert info["keyframe"] == 0
            seen.append(info["changed"])
        assert seen == sorted(seen, reverse=True) and seen[-1] == 0
        if density == 0.0:
            assert seen[0] == 0


@pytest.mark.parametrize("w,h", [(1100, 3), (33, 70), (512, 5)], ids=["1100x3", "33x70", "512x5-row-end-on-a-tile-boundary"])
def test_hook_runs_and_gap_windows_across_the_tile_and_lane_boundaries(enc, w, h):
    rng = np.random.default_rng(w + h)
    shown = _image(rng, h, w)
    groups = [(1023, 1024), (1021, 1022, 1023, 1024, 1025, 1026), (1022, 1025), (1023, 1025), (1020, 1024, 1028), (1015, 1024), (1016, 1025), (1014, 1024),
              (1019, 1020, 1029), (1023,), (1024,), (2047, 2048), (2044, 2051)]
    for cells in groups:
        cells = [c for c in cells if c < w * h]
        cur = shown.copy()
        for k, c in enumerate(cells):          # the top or the bottom half-cell moves by 4: changed under tolerance 3, not under 255
            at = cur[2 * (c // w) + k % 2, c % w]
            at[k % 3] = at[k % 3] + 4 if at[k % 3] < 200 else at[k % 3] - 4
        for gap in (0, 1, 2, 8):
            _, info, _ = check(enc, shown, cur, w, h, gap=gap, tol=3, what=(w, h, cells, gap))
            assert info["changed"] == len(cells)
    if w == 512:          # (511, 1) and (0, 2) are cells 1023 and 1024: two runs whatever the gap
        cur = shown.copy()
        cur[2 * 1, 511, :3], cur[2 * 2 + 1, 0, :3] = (250, 251, 252), (253, 254, 255)
        got, info, _ = check(enc, shown, cur, w, h, gap=8)
        assert info == dict(keyframe=0, changed=2, emitted=3, runs=3) and b"\x1b[2;512H" in got and b"\x1b[3;1H" in got


def test_hook_four_digit_rows_and_columns(enc):
    rng = np.random.default_rng(1001)
    for w, h, cells, tokens in [(3, 1001, [(1000, 0), (999, 0)], [b"\x1b[1001;1H", b"\x1b[1000;1H"]),
                                (1001, 3, [(1, 1000), (0, 999)], [b"\x1b[2;1001H", b"\x1b[1;1000H"])]:
        shown, cur = _frames(rng, h, w, 0.5)
        for y, x in cells:
            cur[2 * y:2 * y + 2, x, :3], shown[2 * y:2 * y + 2, x, :3] = (1, 2, 3), (30, 40, 50)
            if x > 0:
                shown[2 * y:2 * y + 2, x - 1] = cur[2 * y:2 * y + 2, x - 1]
        got, _, _ = check(enc, shown, cur, w, h, gap=0, what=(w, h))
        assert all(t in got for t in tokens), (w, h)


def test_hook_without_shown_is_the_full_stream(enc):
    rng = np.random.default_rng(77)
    _, p = _frames(rng, 11, 20, 1.0)
    for cw, ch, vp, clear in [(21, 11, (0, 0), False), (31, 17, (5, 3), True), (1100, 3, (0, 0), False)]:
        got, info, new = hook_delta(enc, None, p, cw, ch, vp, 2, 14, clear, gap=3, tol=2)
        S.assert_stream(got, R.stream(p, cw, ch, vp, 2, 14, clear), (cw, ch, vp, clear))
        S.assert_stream(got, hook_stream(enc, p, cw, ch, vp, 2, 14, clear), "the full stream's hook")
        assert info == dict(keyframe=1, changed=0, emitted=0, runs=0)
        assert (new[..., :3] == p[..., :3]).all() and (new[..., 3] == 255).all()
    got, info, new = hook_delta(enc, p, p, 21, 11, clear=True)          # clear_screen: a keyframe whatever shown is
    S.assert_stream(got, R.stream(p, 21, 11, clear=True), "clear")
    assert info["keyframe"] == 1


def test_hook_chained_frames_compare_against_what_is_shown(enc):
    """out_shown fed back as shown: a cell that rises by 1 a frame under tolerance 2 is rewritten on every third frame"""
    rng = np.random.default_rng(5)
    base = _image(rng, 3, 9)
    base[2, 4, 0] = 100
    shown = dev_shown = None
    screen, emitted_at = R.Screen(10, 3), []
    for k in range(10):
        cur = base.copy(); cur[2, 4, 0] = 100 + k
        got, info, dev_shown = hook_delta(enc, dev_shown, cur, 10, 3, gap=0, tol=2)
        want, winfo, shown = R.delta(shown, cur, 10, 3, gap=0, tol=2)
        S.assert_stream(got, want, k)
        assert info == winfo and (dev_shown == shown).all()
        if k and info["changed"]:
            emitted_at.append(k)
        screen.feed(got)
        assert R.within(screen, R.Screen(10, 3).feed(R.stream(cur, 10, 3)), 2)
    assert emitted_at == [3, 6, 9]


def test_hook_random_image_641x181(enc):
    rng = np.random.default_rng(181)
    shown, cur = _frames(rng, 180, 640, 1 / 8)
    _, info, _ = check(enc, shown, cur, 641, 181, gap=1, tol=2, what="640x180 in 641x181")
    assert info["runs"] > 1000 and info["emitted"] > info["changed"]
    check_stream(enc, cur, 641, 181, what="640x180 in 641x181, full")


def test_hook_refusals(enc):
    p = np.zeros((4, 3, 4), np.uint8)
    cap = RaytraceRenderer.ansi_rgb_stream_bound(3, 2, enc.L)
    out, n, info = np.zeros(cap, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)()
    fn = enc.L.ycge_test_ansi_rgb_delta
    fn.restype, fn.argtypes = abi.ANSI_RGB_HOOK_PROTOTYPES["ycge_test_ansi_rgb_delta"]
    for gap, tol, c, words in [(3, 256, cap, [b"tolerance 256"]), (3, -1, cap, [b"tolerance -1"]), (9, 0, cap, [b"merge_gap 9"]),
                               (3, 0, cap - 1, [b"capacity %d" % (cap - 1), b"bound %d" % cap, b"ycge_ansi_rgb_stream_bound"])]:
        rc = fn(enc.ctx, p.ctypes.data_as(U8P), p.ctypes.data_as(U8P), 3, 2, 3, 2, 0, 0, 7, 0, 0, gap, tol, out.ctypes.data_as(U8P), c, C.byref(n), info, None)
        msg = enc.L.ycge_last_error(enc.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), (gap, tol, c, msg)
    assert not out.any() and n.value == 0 and list(info) == [0, 0, 0, 0]
    # a console whose 24-bit bound reaches 2^32 is refused although its 256-colour bound does not
    big = C.c_size_t(0)
    assert enc.L.ycge_ansi_rgb_stream_bound(10500, 10500, C.byref(big)) == 0 and big.value >= 2 ** 32 > RaytraceRenderer.ansi_stream_bound(10500, 10500, enc.L)
    rc = fn(enc.ctx, None, p.ctypes.data_as(U8P), 3, 2, 10500, 10500, 0, 0, 7, 0, 0, 3, 0, out.ctypes.data_as(U8P), C.c_size_t(big.value), C.byref(n), info, None)
    assert rc == abi.YCGE_ERR_INVALID_ARG and b"2^32" in enc.L.ycge_last_error(enc.ctx)


# ------------------------------------------------------------------------------------------------------------- 2: frames
FRAME_CASES = [c for c in S.FRAME_CASES if c[0] in (1, 2, 5)]
FRAME_IDS = [f"c{c[0]}-{c[1]}x{c[2]}-ss{c[3]}" for c in FRAME_CASES]


@pytest.mark.parametrize("n,w,h,ss", FRAME_CASES, ids=FRAME_IDS)
def test_full_frames_equal_the_plain_frame_and_the_restatement(product_lib, n, w, h, ss):
    a, b, pose = S.twins(n, w, h, ss)
    try:
        geometries = [(w + 1, h + 1, (0, 0), 7, 0, True), (w + 1, h, (0, 0), 7, 0, False), (w, h, (-2, 1), 15, 1, False)]
        for k, (cw, ch, vp, fg, bg, clear) in enumerate(geometries):
            S.move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, s2 = b.TryFlipAndBlitAnsiRgb(cw, ch, vp, fg, bg, clear, sdr=True)
            assert pu.bits_equal(sdr, s2), (n, k)
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
            S.assert_stream(stream, R.frame_stream(s2, cw, ch, vp, fg, bg, clear), f"config {n} frame {k}")
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("tol", [0, 2])
@pytest.mark.parametrize("n,w,h,ss", FRAME_CASES, ids=FRAME_IDS)
def test_delta_frames_equal_the_plain_frame_the_restatement_and_the_terminal(product_lib, n, w, h, ss, tol):
    a, b, pose = S.twins(n, w, h, ss)
    try:
        cw, ch, gap = w + 1, h, 1                                  # the product's console: one column wider than the framebuffer
        screen, shown = R.Screen(cw, ch), None
        for k, cam in enumerate([0, 0, 0, 1, 1, 1]):               # at rest for three frames, moved, at rest again
            S.move((a, b), pose, cam)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, info, s2 = b.TryFlipAndBlitAnsiRgbDelta(cw, ch, merge_gap=gap, tolerance=tol, sdr=True)
            assert pu.bits_equal(sdr, s2), (n, k)
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
            full = R.frame_stream(s2, cw, ch)
            want, winfo, shown = R.frame_delta(shown, s2, cw, ch, gap=gap, tol=tol)
            S.assert_stream(stream, want, f"config {n} frame {k}")
            assert info == winfo and info["keyframe"] == int(k == 0), (n, k, info, winfo)
            if k == 0:
                S.assert_stream(stream, full, f"config {n}: the first stream is a keyframe")
            assert len(stream) <= len(full)
            screen.feed(stream)
            if tol == 0:
                assert screen.state() == R.Screen(cw, ch).feed(full).state(), (n, k)
            assert R.within(screen, R.Screen(cw, ch).feed(full), tol), (n, k)
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


def step(g, shown, cw=CW, ch=CH, keyframe_expected=False, what="", **kw):
    """one 24-bit delta frame of g, held to the restatement against `shown` (what the terminal displays) or to the keyframe; -> the new shown"""
    kw.setdefault("merge_gap", 1)
    kw.setdefault("tolerance", 1)
    stream, info, s = g.TryFlipAndBlitAnsiRgbDelta(cw, ch, sdr=True, **kw)
    want, winfo, new = R.frame_delta(None if keyframe_expected else shown, s, cw, ch, kw.get("viewport", (0, 0)), kw.get("default_fg", 7), kw.get("default_bg", 0),
                                     kw["merge_gap"], kw["tolerance"], kw.get("clear_screen", False))
    S.assert_stream(stream, want, what)
    assert info == winfo and info["keyframe"] == int(keyframe_expected), (what, info, winfo)
    return new


def step256(g, last, keyframe_expected, what=""):
    """one 256-colour delta frame, held to its restatement; -> its SDR"""
    stream, info, s = g.TryFlipAndBlitAnsiDelta(CW, CH, merge_gap=1, sdr=True)
    want, winfo = D.frame_delta(None if keyframe_expected else last, s, CW, CH, gap=1)
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
    g.Resize(96, 30, 1)                                            # (to the same size: the state is gone all the same)
    step(g, s, 97, 30, keyframe_expected=True, what="after Resize to the same size")


def test_a_changed_viewport_or_default_makes_the_next_call_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    s = step(g, s, viewport=(1, 0), keyframe_expected=True, what="viewport")
    s = step(g, s, viewport=(1, 0), what="delta at the new viewport")
    s = step(g, s, viewport=(1, 0), default_bg=4, keyframe_expected=True, what="default colour")
    s = step(g, s, CW + 1, CH, viewport=(1, 0), default_bg=4, keyframe_expected=True, what="console")
    s = step(g, s, CW + 1, CH, viewport=(1, 0), default_bg=4, merge_gap=5, what="another merge_gap is no other geometry")
    step(g, s, CW + 1, CH, viewport=(1, 0), default_bg=4, tolerance=4, what="nor is another tolerance")


def test_keyframe_and_clear_screen_give_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s, keyframe=True, keyframe_expected=True, what="keyframe = 1")
    s = step(g, s, what="delta")
    stream, info = g.TryFlipAndBlitAnsiRgbDelta(CW, CH, clear_screen=True, merge_gap=1)
    assert info["keyframe"] == 1 and stream.startswith(b"\x1b[2J\x1b[H\x1b[1;1H\x1b[38;2;")
    s = step(g, s, clear_screen=True, keyframe_expected=True, what="clear_screen")
    step(g, s, what="delta again")


def test_an_interleaved_full_stream_of_either_family_makes_the_next_call_a_keyframe(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    g.TryFlipAndBlit()                                             # (a plain frame shows the terminal nothing)
    S.move([g], pose, 1)
    s = step(g, s, what="a delta against what the terminal shows, two frames back")
    g.TryFlipAndBlitAnsiRgb(CW, CH)
    s = step(g, s, keyframe_expected=True, what="after TryFlipAndBlitAnsiRgb")
    s = step(g, s, what="delta")
    g.TryFlipAndBlitAnsi(CW, CH)
    s = step(g, s, keyframe_expected=True, what="after the 256-colour TryFlipAndBlitAnsi")
    step(g, s, what="delta")


def test_the_two_delta_families_invalidate_each_other(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    p = step256(g, None, True, "a 256-colour delta after 24-bit ones is a keyframe")
    p = step256(g, p, False, "256-colour delta")
    s = step(g, s, keyframe_expected=True, what="a 24-bit delta after a 256-colour one")
    s = step(g, s, what="24-bit delta")
    g.TryFlipAndBlitAnsiRgb(CW, CH)                                # the converse of the old file's rule: a 24-bit full stream ...
    p = step256(g, p, True, "... makes the next 256-colour delta a keyframe")
    step256(g, p, False, "256-colour delta again")


def _call(g, cw, ch, out, cap, n, info=None, sdr=None, gap=1, tol=1, keyframe=0, clear=0, ctx=None):
    return g.L.ycge_render_frame_ansi_rgb_delta(ctx if ctx is not None else g.ctx, cw, ch, 0, 0, 7, 0, clear, gap, tol, keyframe, out.ctypes.data_as(U8P), cap,
                                                C.byref(n), info, sdr.ctypes.data_as(C.POINTER(C.c_float)) if sdr is not None else None, None)


def _call_full(g, cw, ch, out, cap, n, ctx=None):
    return g.L.ycge_render_frame_ansi_rgb(ctx if ctx is not None else g.ctx, cw, ch, 0, 0, 7, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), None, None)


def test_a_refused_call_leaves_shown_alone(one):
    g, pose = one
    s = step(g, None, keyframe_expected=True)
    s = step(g, s)
    frame = g.stats.frame
    cap = RaytraceRenderer.ansi_rgb_stream_bound(CW, CH, g.L)
    out, n, info = np.zeros(cap, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)()
    for kw, words in [(dict(tol=256), [b"tolerance 256"]), (dict(tol=-1), [b"tolerance -1"]), (dict(gap=9), [b"merge_gap 9"]),
                      (dict(cap=cap - 1), [b"capacity %d" % (cap - 1), b"bound %d" % cap]),
                      (dict(cap=RaytraceRenderer.ansi_stream_bound(CW, CH, g.L)), [b"ycge_ansi_rgb_stream_bound"])]:
        rc = _call(g, CW, CH, out, kw.get("cap", cap), n, info, gap=kw.get("gap", 1), tol=kw.get("tol", 1))
        msg = g.L.ycge_last_error(g.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), (kw, rc, msg)
    assert _call_full(g, CW, CH, out, cap - 1, n) == abi.YCGE_ERR_INVALID_ARG          # (a refused full stream shows the terminal nothing either)
    assert not out.any() and n.value == 0 and list(info) == [0, 0, 0, 0]
    S.move([g], pose, 2)
    step(g, s, what="the next delta is against what the terminal showed before the refusals")
    assert g.stats.frame == frame + 1


def test_a_video_delta_follows_a_ray_traced_one_on_the_shared_context(one):
    g, pose = one
    v = VideoRenderer(renderer=g)
    rng = np.random.default_rng(3)
    movie = rng.integers(0, 256, (36, 64, 3)).astype(np.uint8)
    s = step(g, None, keyframe_expected=True)
    stream, info, vs = v.TryFlipAndBlitAnsiRgbDelta(movie, CW, CH, merge_gap=2, tolerance=1, sdr=True)
    want, winfo, s = R.frame_delta(s, vs, CW, CH, gap=2, tol=1)
    S.assert_stream(stream, want, "video against the ray-traced frame")
    assert info == winfo and info["keyframe"] == 0 and info["changed"] > 0
    stream, info = v.TryFlipAndBlitAnsiRgbDelta(movie, CW, CH, merge_gap=2, tolerance=0)
    want, winfo, s = R.frame_delta(s, vs, CW, CH, gap=2, tol=0)
    assert (stream, info) == (want, winfo)
    stream, info = v.TryFlipAndBlitAnsiRgbDelta(movie, CW, CH, merge_gap=2, tolerance=0)         # the same picture, all of it shown: the last cell alone
    assert info == dict(keyframe=0, changed=0, emitted=1, runs=1)
    s = step(g, s, what="ray-traced against the video frame")
    full, vs2 = v.TryFlipAndBlitAnsiRgb(movie, CW, CH, sdr=True)
    S.assert_stream(full, R.frame_stream(vs2, CW, CH), "the video's full 24-bit stream")
    assert pu.bits_equal(vs, vs2)
    step(g, s, keyframe_expected=True, what="after the video's full stream")


def test_pageable_and_page_locked_destinations(one):
    g, pose = one
    cap = RaytraceRenderer.ansi_rgb_stream_bound(CW, CH, g.L)
    shown = None
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
        want, winfo, shown = R.frame_delta(shown, s2, CW, CH, gap=1, tol=1)
        S.assert_stream(out[:n.value].tobytes(), want, f"{form} {k}")
        assert dict(zip(R.INFO, info)) == winfo
    for form in ("pageable", "locked"):
        out = g._page_locked_zeros((cap + 64,), np.uint8)[0] if form == "locked" else np.zeros(cap + 64, np.uint8)
        out[...] = CANARY
        n = C.c_size_t(0)
        s2 = np.zeros((45, 80, 2, 3), np.float32)
        g._check(g.L.ycge_render_frame_ansi_rgb(g.ctx, CW, CH, 0, 0, 7, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), s2.ctypes.data_as(C.POINTER(C.c_float)), None))
        assert (out[n.value:] == CANARY).all()
        S.assert_stream(out[:n.value].tobytes(), R.frame_stream(s2, CW, CH), f"full, {form}")


def test_a_peer_context_is_refused_and_its_root_streams(product_lib):
    a, b, pose = S.twins(2, 160, 45, 1, devices=[0, 0, 0])
    try:
        fn = b.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, C.c_int32]
        peer = fn(b.ctx, 0)
        assert peer
        cap = RaytraceRenderer.ansi_rgb_stream_bound(161, 45, b.L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        for rc in (_call(b, 161, 45, out, cap, n, ctx=peer), _call_full(b, 161, 45, out, cap, n, ctx=peer)):
            assert rc == abi.YCGE_ERR_INVALID_ARG and b"driven by their root" in b.L.ycge_last_error(peer)
        assert not out.any() and n.value == 0
        shown = None
        for k in range(3):
            S.move((a, b), pose, k)
            sdr = a.TryFlipAndBlit(want_sdr=True)
            stream, info, s2 = b.TryFlipAndBlitAnsiRgbDelta(161, 45, merge_gap=0, tolerance=1, sdr=True)
            assert pu.bits_equal(sdr, s2), k
            want, winfo, shown = R.frame_delta(shown, s2, 161, 45, gap=0, tol=1)
            S.assert_stream(stream, want, f"peer push {k}")
            assert info == winfo
    finally:
        a.close(); b.close()


def test_the_lean_slab_refusal_is_that_of_the_256_colour_streams(product_lib):
    cfg = abi.default_config()
    cfg.multi_device_exchange = abi.EXCHANGE_RCCL
    sc, w, h, ss, pose = scenes.config_scene(1)
    lean = RaytraceRenderer(flatten(sc), 80, 45, pose["fov"], 1, cfg=cfg, devices=[0], slab_albedo=False)
    try:
        cap = RaytraceRenderer.ansi_rgb_stream_bound(CW, CH, lean.L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        assert S._call(lean, CW, CH, out, cap, n) == abi.YCGE_ERR_INVALID_ARG
        msg = lean.L.ycge_last_error(lean.ctx)
        assert b"lean slabs" in msg
        for rc in (_call(lean, CW, CH, out, cap, n), _call_full(lean, CW, CH, out, cap, n)):
            assert rc == abi.YCGE_ERR_INVALID_ARG and lean.L.ycge_last_error(lean.ctx) == msg
        assert not out.any() and n.value == 0
    finally:
        lean.close()
