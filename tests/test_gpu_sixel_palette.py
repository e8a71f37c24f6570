"""The adaptive sixel palette on the GPU: the palette stage and the 256-register encoder alone through the two hooks on the planes of
tests/sixel_palette_planes.py, against tests/sixel_palette_restatement.py - registers, palette, percentages, count and stream, byte for
byte, the stream decoded by the independent interpreter; the kept palette; a traced frame and a video source through the exports beside a
twin context that takes the cube calls' RGBA plane through the host functions; the delta state, the refusals, the host route, and the
cube calls behind a _palette call.  Every comparison is exact, every stream is checked to its length with a canary behind it."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import parity_util as pu
import sixel_palette_planes as PP
import sixel_palette_restatement as R
import test_gpu_ansi_stream as S
import video_quadrant_inputs as I
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VideoRenderer

pytestmark = pytest.mark.gpu
U8P = C.POINTER(C.c_uint8)
ROOT = Path(__file__).resolve().parents[1]
EXPORTS = ("ycge_sixel_palette_stream_bound", "ycge_render_frame_sixel_palette", "ycge_video_blit_sixel_palette", "ycge_render_frame_pixels_palette",
           "ycge_video_blit_pixels_palette", "ycge_sixel_palette_host", "ycge_sixel_encode_palette_host", "ycge_test_sixel_palette", "ycge_test_sixel_palette_stream")


@pytest.fixture(scope="module")
def lib(product_lib):
    """the exports, looked up first: a library without them fails here, it does not skip"""
    for n in EXPORTS:
        assert getattr(product_lib, n) is not None
    return product_lib


@pytest.fixture(scope="module")
def enc(lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


def hook_palette(g, rgba, hold=False):
    """ycge_test_sixel_palette on an RGBA plane (H, W, 4) -> (index, palette, pct, n); nothing past an output was written"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    H, W = rgba.shape[:2]
    fn = g.L.ycge_test_sixel_palette
    fn.restype, fn.argtypes = abi.SIXEL_PALETTE_HOOK_PROTOTYPES["ycge_test_sixel_palette"]
    index, palette, pct, n = np.full(W * H + 64, PP.CANARY, np.uint8), np.full(1024 + 64, PP.CANARY, np.uint8), np.full(768 + 64, PP.CANARY, np.uint8), C.c_int32(-1)
    g._check(fn(g.ctx, rgba.ctypes.data_as(U8P), W, H, int(hold), index.ctypes.data_as(U8P), palette.ctypes.data_as(U8P), pct.ctypes.data_as(U8P), C.byref(n)))
    for a, size in ((index, W * H), (palette, 1024), (pct, 768)):
        assert (a[size:] == PP.CANARY).all(), "bytes past an output were written"
    return index[:W * H].reshape(H, W), palette[:1024].reshape(256, 4), pct[:768].reshape(256, 3), n.value


def hook_stream(g, rgba, viewport=(0, 0), clear=False, hold=False):
    """ycge_test_sixel_palette_stream -> the stream; no byte at or past its length was written"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    H, W = rgba.shape[:2]
    fn = g.L.ycge_test_sixel_palette_stream
    fn.restype, fn.argtypes = abi.SIXEL_PALETTE_HOOK_PROTOTYPES["ycge_test_sixel_palette_stream"]
    cap = R.bound(W, H)
    out, n = np.full(cap + 64, PP.CANARY, np.uint8), C.c_size_t(0)
    g._check(fn(g.ctx, rgba.ctypes.data_as(U8P), W, H, viewport[0], viewport[1], int(clear), int(hold), out.ctypes.data_as(U8P), cap, C.byref(n)))
    assert n.value <= cap and (out[n.value:] == PP.CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes()


def assert_palette(got, want, what):
    index, palette, pct, n = got
    _, w_index, w_palette, w_pct, w_n, _ = want
    assert n == w_n, (what, n, w_n)
    assert np.array_equal(palette, w_palette) and np.array_equal(pct, w_pct), (what, np.argwhere(palette != w_palette)[:4])
    assert np.array_equal(index, w_index), (what, np.argwhere(index != w_index)[:4])


# ------------------------------------------------------------------------------------------------------------- 1: the kernels alone
@pytest.mark.parametrize("name", sorted(PP.PLANES))
def test_hooks_on_the_planes(enc, name):
    rgba = PP.plane(name)
    assert_palette(hook_palette(enc, rgba), PP.expected(name), name)
    for k in range(2):
        want = PP.expected(name, k)
        got = hook_stream(enc, rgba, PP.VIEWPORTS[k % 3], bool(k & 1))
        S.assert_stream(got, want[0], (name, k))
        shown, vp, clear, defined = R.shown(got)
        assert defined == want[4] and vp == PP.VIEWPORTS[k % 3] and clear == bool(k & 1)
        assert np.array_equal(shown, want[3].astype(np.int64)[want[1]]), name


def test_the_kept_palette(lib):
    first, second = PP.hold_pair()
    built = R.stream(first)
    held = (built[5], built[2], built[3], built[4])
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    try:
        # hold with nothing kept: built from the picture at hand
        assert_palette(hook_palette(g, first, hold=True), built, "hold with nothing kept")
        # the second picture through the first's palette, pixels in bins the first left empty among them; and its stream
        assert_palette(hook_palette(g, second, hold=True), R.stream(second, held=held), "hold")
        S.assert_stream(hook_stream(g, second, (2, 1), True, hold=True), R.stream(second, (2, 1), True, held)[0], "the held stream")
        # hold = 0 replaces it
        own = R.stream(second)
        assert_palette(hook_palette(g, second), own, "rebuilt")
        assert_palette(hook_palette(g, first, hold=True), R.stream(first, held=(own[5], own[2], own[3], own[4])), "the first through the second's")
    finally:
        g.close()


def test_hook_refusals_keep_the_palette(enc):
    first, second = PP.hold_pair()
    built = R.stream(first)
    hook_palette(enc, first)
    fn = enc.L.ycge_test_sixel_palette_stream
    fn.restype, fn.argtypes = abi.SIXEL_PALETTE_HOOK_PROTOTYPES["ycge_test_sixel_palette_stream"]
    rgba = np.ascontiguousarray(second)
    H, W = rgba.shape[:2]
    cap = R.bound(W, H)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    p, o = rgba.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
    for args, word in [((None, W, H, 0, 0, 0, 0, o, cap, C.byref(n)), b""), ((p, W, H, 0, 0, 0, 2, o, cap, C.byref(n)), b"hold 2"), ((p, W, H, 0, 0, 0, -1, o, cap, C.byref(n)), b"hold -1"),
                       ((p, W, H, -1, 0, 0, 0, o, cap, C.byref(n)), b"(-1, 0)"), ((p, W, H, 0, 0, 0, 0, o, cap - 1, C.byref(n)), b"capacity %d" % (cap - 1)),
                       ((p, 0, H, 0, 0, 0, 0, o, cap, C.byref(n)), b""), ((p, 4097, 4096, 0, 0, 0, 0, o, cap, C.byref(n)), b"4097 x 4096"), ((p, W, H, 0, 0, 0, 0, None, cap, C.byref(n)), b"NULL")]:
        assert fn(enc.ctx, *args) == abi.YCGE_ERR_INVALID_ARG and word in enc.L.ycge_last_error(enc.ctx)
    assert not out.any() and n.value == 0
    assert_palette(hook_palette(enc, second, hold=True), R.stream(second, held=(built[5], built[2], built[3], built[4])), "the kept palette survived the refusals")


# ------------------------------------------------------------------------------------------------------------- 2: frames and video
def host_stream(L, rgba, vp, clear):
    """the twin's road: the cube call's RGBA plane through ycge_sixel_palette_host and ycge_sixel_encode_palette_host"""
    import test_sixel_palette_cpu as T
    index, palette, pct, n = T.host_palette(L, rgba)
    return T.host_encode(L, index, pct, n, vp, clear), palette, n


def palette_call(g, vp=(2, 1), clear=0, hold=0):
    """ycge_render_frame_sixel_palette into a buffer of the bound's size with a canary behind it: (bytes, palette, n, sdr)"""
    W, H = g.fbW * g.ss, 2 * g.fbH * g.ss
    cap = R.bound(W, H)
    out, n = np.full(cap + 64, PP.CANARY, np.uint8), C.c_size_t(0)
    palette, count, sdr = np.zeros((256, 4), np.uint8), C.c_int32(-1), np.zeros((g.fbH, g.fbW, 2, 3), np.float32)
    g._check(g.L.ycge_render_frame_sixel_palette(g.ctx, vp[0], vp[1], clear, hold, out.ctypes.data_as(U8P), cap, C.byref(n), palette.ctypes.data_as(U8P), C.byref(count),
                                                 sdr.ctypes.data_as(C.POINTER(C.c_float)), C.byref(g.stats)))
    assert n.value <= cap and (out[n.value:] == PP.CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), palette, count.value, sdr


def test_a_frame_beside_a_twin(lib):
    """config 1 at 7 x 3 chexels, super_sample 2: the stream is the host functions' on the twin's RGBA plane, the SDR and the frame state are
    ycge_render_frame's; the second frame holds the first's palette"""
    a, b, pose = S.twins(1, 7, 3, 2)
    try:
        want = a.TryFlipAndBlitPixels(rgba=True, index=False, sdr=True)
        stream, palette, n, sdr = palette_call(b, (2, 1), 1, 0)
        first = R.stream(want["rgba"], (2, 1), True)
        w_stream, w_palette, w_n = host_stream(lib, want["rgba"], (2, 1), True)
        S.assert_stream(stream, w_stream, "frame 1")
        assert w_stream == first[0], "the host functions are the restatement's"
        assert n == w_n and np.array_equal(palette, w_palette)
        assert pu.bits_equal(sdr, want["sdr"]) and a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure
        shown, *_ = R.shown(stream)
        assert np.array_equal(shown, first[3].astype(np.int64)[first[1]])
        # frame 2, the camera moved, through the kept palette; the planes call beside it
        S.move((a, b), pose, 3)
        want = a.TryFlipAndBlitPixels(rgba=True, index=False, sdr=True)
        stream, palette, n, sdr = palette_call(b, (2, 1), 0, 1)
        held = (first[5], first[2], first[3], first[4])
        S.assert_stream(stream, R.stream(want["rgba"], (2, 1), False, held)[0], "frame 2, held")
        assert n == first[4] and np.array_equal(palette, first[2]) and pu.bits_equal(sdr, want["sdr"])
        S.move((a, b), pose, 5)
        want = a.TryFlipAndBlitPixels(rgba=True, index=False, sdr=True)
        planes = b.TryFlipAndBlitPixelsPalette(sdr=True)
        own = R.stream(want["rgba"])
        assert np.array_equal(planes["rgba"], want["rgba"]) and np.array_equal(planes["index"], own[1]) and planes["count"] == own[4]
        assert np.array_equal(planes["palette"], own[2]) and pu.bits_equal(planes["sdr"], want["sdr"])
        only = b.L.ycge_render_frame_pixels_palette(b.ctx, None, None, None, 0, None, None, None)
        assert only == abi.YCGE_ERR_INVALID_ARG
        a.TryFlipAndBlit(want_sdr=True)
        count = C.c_int32(0)
        b._check(b.L.ycge_render_frame_pixels_palette(b.ctx, None, None, None, 1, None, C.byref(count), C.byref(b.stats)))
        assert count.value == own[4] and a.stats.frame == b.stats.frame
        assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))
    finally:
        a.close(); b.close()


def test_a_video_source_beside_a_twin(lib):
    sw, sh, bpp, fw, fh, ss = 64, 48, 3, 20, 5, 2
    f = I.drawn(sw, sh, bpp)
    with VideoRenderer(fw, fh, ss, lib=lib) as a, VideoRenderer(fw, fh, ss, lib=lib) as b:
        want = a.TryFlipAndBlitPixels(f, rgba=True, index=False, sdr=True)
        stream, palette, n, sdr = b.TryFlipAndBlitSixelPalette(f, (3, 2), clear_screen=True, sdr=True)
        own = R.stream(want["rgba"], (3, 2), True)
        S.assert_stream(stream, host_stream(lib, want["rgba"], (3, 2), True)[0], "video")
        S.assert_stream(stream, own[0], "video, the restatement")
        assert n == own[4] and np.array_equal(palette, own[2]) and pu.bits_equal(sdr, want["sdr"])
        assert len(stream) <= RaytraceRenderer.sixel_palette_stream_bound(fw * ss, 2 * fh * ss, lib) == R.bound(fw * ss, 2 * fh * ss)
        # another source through the kept palette, and the planes
        f2 = I.noise(sw, sh, bpp)
        want2 = a.TryFlipAndBlitPixels(f2, rgba=True, index=False)
        held = (own[5], own[2], own[3], own[4])
        S.assert_stream(b.TryFlipAndBlitSixelPalette(f2, (3, 2), hold=True)[0], R.stream(want2["rgba"], (3, 2), False, held)[0], "video, held")
        planes = b.TryFlipAndBlitPixelsPalette(f2, sdr=True)
        own2 = R.stream(want2["rgba"])
        assert np.array_equal(planes["rgba"], want2["rgba"]) and np.array_equal(planes["index"], own2[1]) and planes["count"] == own2[4] and np.array_equal(planes["palette"], own2[2])


# ------------------------------------------------------------------------------------------------------------- 3: state and refusals
FBW, FBH, SS, VP, CW, CH = 20, 6, 2, (2, 1), 24, 8


@pytest.fixture()
def pair(lib):
    a, b, pose = S.twins(1, FBW, FBH, SS)
    yield a, b, pose
    a.close(); b.close()


def test_an_adaptive_stream_invalidates_the_delta_state(pair):
    _, g, _ = pair
    sixel_key = lambda: g.TryFlipAndBlitSixelDelta(VP)[1][0]
    ansi_key = lambda: g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)[1]["keyframe"]
    assert sixel_key() == 1 and sixel_key() == 0
    g.TryFlipAndBlitPixelsPalette()
    assert sixel_key() == 0, "the planes call leaves the state alone"
    g.TryFlipAndBlitSixelPalette(VP)
    assert sixel_key() == 1 and sixel_key() == 0, "an adaptive stream paints over the cube's picture"
    assert ansi_key() == 1 and ansi_key() == 0
    g.TryFlipAndBlitPixelsPalette(hold=True)
    assert ansi_key() == 0
    g.TryFlipAndBlitSixelPalette(VP, hold=True)
    assert ansi_key() == 1, "an adaptive stream paints over the cells"
    v = VideoRenderer(renderer=g)
    f = I.drawn(40, 30, 3)
    assert v.TryFlipAndBlitSixelDelta(f, VP)[1][0] == 1 and v.TryFlipAndBlitSixelDelta(f, VP)[1][0] == 0
    v.TryFlipAndBlitPixelsPalette(f)
    assert v.TryFlipAndBlitSixelDelta(f, VP)[1][0] == 0
    v.TryFlipAndBlitSixelPalette(f, VP)
    assert v.TryFlipAndBlitSixelDelta(f, VP)[1][0] == 1


def test_refusals_leave_the_context_the_delta_state_and_the_kept_palette(pair):
    a, g, pose = pair
    L = g.L
    key = lambda: g.TryFlipAndBlitSixelDelta(VP)[1][0]
    first = a.TryFlipAndBlitPixels(rgba=True, index=False)["rgba"]
    g.TryFlipAndBlitPixelsPalette()
    built = R.stream(first)
    assert key() == 1 and key() == 0
    a.TryFlipAndBlit(want_sdr=True); a.TryFlipAndBlit(want_sdr=True)
    frame0 = g.stats.frame
    history = g.read(abi.BUF_TAA_HISTORY).copy()
    W, H = FBW * SS, 2 * FBH * SS
    cap = R.bound(W, H)
    out, n, palette, count = np.zeros(cap, np.uint8), C.c_size_t(0), np.zeros((256, 4), np.uint8), C.c_int32(-5)
    p, q = out.ctypes.data_as(U8P), palette.ctypes.data_as(U8P)
    call = lambda vx=0, vy=0, hold=0, o=p, c=cap, ln=C.byref(n): L.ycge_render_frame_sixel_palette(g.ctx, vx, vy, 0, hold, o, c, ln, q, C.byref(count), None, None)
    src = np.ascontiguousarray(I.drawn(40, 30, 3))
    video = lambda hold=0, bpp=3, c=cap: L.ycge_video_blit_sixel_palette(g.ctx, src.ctypes.data_as(U8P), 40, 30, bpp, 0, 0, 0, hold, p, c, C.byref(n), q, C.byref(count), None)
    for fn, name, words in [(lambda: call(o=None), b"ycge_render_frame_sixel_palette", [b"NULL"]), (lambda: call(ln=None), b"ycge_render_frame_sixel_palette", [b"NULL"]),
                            (lambda: call(c=cap - 1), b"ycge_render_frame_sixel_palette", [b"capacity %d" % (cap - 1)]),
                            (lambda: call(vx=-1), b"ycge_render_frame_sixel_palette", [b"(-1, 0)"]), (lambda: call(vy=-7), b"ycge_render_frame_sixel_palette", [b"(0, -7)"]),
                            (lambda: call(hold=2), b"ycge_render_frame_sixel_palette", [b"hold 2"]), (lambda: call(hold=-1), b"ycge_render_frame_sixel_palette", [b"hold -1"]),
                            (lambda: L.ycge_render_frame_pixels_palette(g.ctx, None, None, None, 3, q, None, None), b"ycge_render_frame_pixels_palette", [b"hold 3"]),
                            (lambda: video(hold=2), b"ycge_video_blit_sixel_palette", [b"hold 2"]), (lambda: video(c=cap - 1), b"ycge_video_blit_sixel_palette", [b"capacity"]),
                            (lambda: video(bpp=2), b"ycge_video_blit_sixel_palette", []),
                            (lambda: L.ycge_video_blit_pixels_palette(g.ctx, src.ctypes.data_as(U8P), 40, 30, 3, None, None, None, 7, q, None), b"ycge_video_blit_pixels_palette", [b"hold 7"])]:
        rc = fn()
        msg = L.ycge_last_error(g.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words) and name in msg, msg
    assert not out.any() and n.value == 0 and not palette.any() and count.value == -5
    assert pu.bits_equal(g.read(abi.BUF_TAA_HISTORY), history)
    assert key() == 0, "a refused call forces no keyframe"
    assert g.stats.frame == frame0 + 1
    a.TryFlipAndBlit(want_sdr=True)
    # the kept palette is the first frame's still
    S.move((a, g), pose, 4)
    want = a.TryFlipAndBlitPixels(rgba=True, index=False)["rgba"]
    got = g.TryFlipAndBlitPixelsPalette(hold=True)
    assert got["count"] == built[4] and np.array_equal(got["palette"], built[2]) and np.array_equal(got["index"], R.remap(want, built[5]))
    # ycge_resize keeps it too: another geometry through the same palette
    g.Resize(FBW + 1, FBH, 1); a.Resize(FBW + 1, FBH, 1)
    want = a.TryFlipAndBlitPixels(rgba=True, index=False)["rgba"]
    got = g.TryFlipAndBlitPixelsPalette(hold=True)
    assert got["count"] == built[4] and np.array_equal(got["index"], R.remap(want, built[5]))


def test_a_peer_context_is_refused(lib):
    a, b, pose = S.twins(2, 160, 45, 2, devices=[0, 0, 0])
    try:
        a.close()
        fn = b.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = abi.HOOK_PROTOTYPES["ycge_debug_peer_context"]
        peer = fn(b.ctx, 0)
        assert peer
        index = np.zeros((180, 320), np.uint8)
        count = C.c_int32(-3)
        assert b.L.ycge_render_frame_pixels_palette(peer, None, None, index.ctypes.data_as(U8P), 0, None, C.byref(count), None) == abi.YCGE_ERR_INVALID_ARG
        cap = RaytraceRenderer.sixel_palette_stream_bound(320, 180, b.L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        assert b.L.ycge_render_frame_sixel_palette(peer, 0, 0, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), None, C.byref(count), None, None) == abi.YCGE_ERR_INVALID_ARG
        assert not index.any() and not out.any() and n.value == 0 and count.value == -3
    finally:
        b.close()


def test_the_cube_calls_behind_a_palette_call(pair):
    """after frames through the new calls, _sixel, _sixel_delta and _ansi_rgb give the bytes of a context that never saw them"""
    a, b, pose = pair
    a.TryFlipAndBlit(want_sdr=True); b.TryFlipAndBlitSixelPalette(VP)
    a.TryFlipAndBlit(want_sdr=True); b.TryFlipAndBlitPixelsPalette(hold=True)
    for k, dither in enumerate((False, True)):
        S.move((a, b), pose, k + 1)
        S.assert_stream(b.TryFlipAndBlitSixel(VP, dither=dither), a.TryFlipAndBlitSixel(VP, dither=dither), ("_sixel", dither))
    for k in range(3):
        S.move((a, b), pose, k // 2)
        sa, ia = a.TryFlipAndBlitSixelDelta(VP)
        sb, ib = b.TryFlipAndBlitSixelDelta(VP)
        S.assert_stream(sb, sa, ("_sixel_delta", k))
        assert ia == ib and ia[0] == (k == 0)
    S.assert_stream(b.TryFlipAndBlitAnsiRgb(CW, CH, VP, 3, 12), a.TryFlipAndBlitAnsiRgb(CW, CH, VP, 3, 12), "_ansi_rgb")
    assert a.stats.frame == b.stats.frame and pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY))


# ------------------------------------------------------------------------------------------------------------- 4: the host route
CHILD = """
import json, sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_sixel_palette as T
print("RESULT " + json.dumps(T.route_streams()))
"""


def route_streams():
    a, b, pose = S.twins(1, 16, 8, 2)
    try:
        a.close()
        first, second = PP.hold_pair()
        out = dict(hook=hook_stream(b, first, (9, 99), True).hex(), held=hook_stream(b, second, (1, 2), False, hold=True).hex())
        frames = []
        for k in range(3):
            S.move((b,), pose, 3 * k)
            stream, palette, n = b.TryFlipAndBlitSixelPalette((1, 2), hold=(k == 1))
            frames.append([stream.hex(), palette.tobytes().hex(), n])
        out["frames"] = frames
        with VideoRenderer(renderer=b) as v:
            stream, palette, n = v.TryFlipAndBlitSixelPalette(I.drawn(64, 48, 3), (1, 2), hold=True)
            out["video"] = [stream.hex(), n]
        return out
    finally:
        b.close()


def test_the_host_route_gives_the_same_bytes(lib):
    want = route_streams()
    env = dict(os.environ, YCGE_SIXEL_HOST="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(tests=str(ROOT / "tests"), root=str(ROOT))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert got == want
