"""The sixel frames on the GPU: the encoder's kernels alone through ycge_test_sixel_stream on drawn and built register planes, byte for byte
against tests/sixel_restatement.py; k_sixel_pixels alone through ycge_test_pixels on inputs no frame produces; the frames of
ycge_render_frame_pixels / _sixel on the Cornell box beside a twin context; the state rules, the refusals and the host fallback.  Every
stream is checked to its exact length, with a canary behind it."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import parity_util as pu
import post_probe_inputs as ppi
import sixel_planes as P
import sixel_restatement as X
import test_gpu_ansi_stream as S
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

pytestmark = pytest.mark.gpu
f32 = np.float32
U8P = C.POINTER(C.c_uint8)
ROOT = Path(__file__).resolve().parents[1]


def _hook(g, name):
    fn = getattr(g.L, name)
    fn.restype, fn.argtypes = abi.SIXEL_HOOK_PROTOTYPES[name]
    return fn


def hook_stream(g, plane, viewport=(0, 0), clear=False):
    """ycge_test_sixel_stream on a register plane (H, W) -> the stream; checks that nothing at or past its length was written"""
    plane = np.ascontiguousarray(plane, np.uint8)
    H, W = plane.shape
    cap = RaytraceRenderer.sixel_stream_bound(W, H, g.L)
    assert cap == X.bound(W, H)
    out, n = np.full(cap + 64, P.CANARY, np.uint8), C.c_size_t(0)
    g._check(_hook(g, "ycge_test_sixel_stream")(g.ctx, plane.ctypes.data_as(U8P), W, H, viewport[0], viewport[1], int(clear), out.ctypes.data_as(U8P), cap, C.byref(n)))
    assert n.value <= cap and (out[n.value:] == P.CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes()


def hook_pixels(g, hdr, fbW, fbH, ss, exposure, dither):
    hdr = np.ascontiguousarray(hdr, f32)
    H, W = 2 * fbH * ss, fbW * ss
    assert hdr.shape == (H, W, 3)
    rgba, index = np.full((H, W, 4), 0x5A, np.uint8), np.full((H, W), 0xEE, np.uint8)
    g._check(_hook(g, "ycge_test_pixels")(g.ctx, hdr.ctypes.data, fbW, fbH, ss, float(exposure), int(dither), rgba.ctypes.data, index.ctypes.data))
    return rgba, index


@pytest.fixture(scope="module")
def enc(product_lib):
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------------------------- 1: the encoder alone
SMALL = (1, 3, 4, 5, 9, 10, 11, 63, 64, 65)
LARGE = (99, 100, 101, 127, 128, 129, 255, 256, 257, 999, 1000, 1001, 4097)


@pytest.mark.parametrize("w", SMALL + LARGE)
def test_encoder_on_drawn_planes(enc, w):
    """widths around the walk's 64-column trips, the run-length digits' steps and the presence tiles (1024 columns); heights around a band"""
    k = 0
    for h in (P.HEIGHTS if w in SMALL else (6, 7)):
        for plane in P.drawn(w, h):
            vp, clear = P.VIEWPORTS[k % 3], bool(k // 3 & 1)
            S.assert_stream(hook_stream(enc, plane, vp, clear), X.encode(plane, vp, clear), (w, h, k))
            k += 1


@pytest.mark.parametrize("name", sorted(P.SEAMS))
def test_encoder_on_built_planes(enc, name):
    plane = P.SEAMS[name]()
    for vp in P.VIEWPORTS:
        for clear in (False, True):
            got = hook_stream(enc, plane, vp, clear)
            S.assert_stream(got, X.encode(plane, vp, clear), (name, vp, clear))
    assert np.array_equal(X.decode(got)[0], plane)


def test_encoder_hook_refusals(enc):
    fn = _hook(enc, "ycge_test_sixel_stream")
    plane = np.zeros((7, 5), np.uint8)
    cap = X.bound(5, 7)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    p, o = plane.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
    bad = plane.copy(); bad[3, 2] = 216
    for args, word in [((None, 5, 7, 0, 0, 0, o, cap, C.byref(n)), b"bad arguments"), ((p, 5, 7, -1, 0, 0, o, cap, C.byref(n)), b"(-1, 0)"),
                       ((p, 5, 7, 0, 0, 0, o, cap - 1, C.byref(n)), b"capacity %d" % (cap - 1)), ((p, 0, 7, 0, 0, 0, o, cap, C.byref(n)), b"0 x 7"),
                       ((bad.ctypes.data_as(U8P), 5, 7, 0, 0, 0, o, cap, C.byref(n)), b"register 216 at pixel 17"), ((p, 5, 7, 0, 0, 0, o, cap, None), b"bad arguments")]:
        assert fn(enc.ctx, *args) == abi.YCGE_ERR_INVALID_ARG and word in enc.L.ycge_last_error(enc.ctx), (word, enc.L.ycge_last_error(enc.ctx))
    assert not out.any() and n.value == 0


# ------------------------------------------------------------------------------------------------------------- 2: the pixel stage alone
def check_pixels(g, hdr, fbw, fbh, ss, exposure, what):
    for dither in (0, 1):
        rgba, index = hook_pixels(g, hdr, fbw, fbh, ss, exposure, dither)
        wrgba, windex = X.pixels(hdr, fbw, fbh, ss, exposure, dither)
        assert np.array_equal(rgba, wrgba), (what, dither, np.argwhere(rgba != wrgba)[:4])
        assert np.array_equal(index, windex), (what, dither, np.argwhere(index != windex)[:4])
    return wrgba


@pytest.mark.parametrize("fbw,fbh,ss", [(1, 1, 1), (7, 3, 2), (257, 3, 1), (5, 2, 4), (3, 2, 3)])
def test_pixels_exactly(enc, fbw, fbh, ss):
    """drawn HDR, then the post probe's special values - NaN, +-inf, negatives, denormals, 1e30, FLT_MAX - in one channel or in all three;
    (1, 1, 1) and (3, 2, 3): pixel counts that are no multiple of the four a lane takes; (257, 3, 1): more than one workgroup"""
    rng = np.random.default_rng([fbw, fbh, ss])
    H, W = fbh * 2 * ss, fbw * ss
    hdr = rng.uniform(0, 2.5, (H, W, 3)).astype(f32)
    hdr[rng.random((H, W)) < 0.1] = 0
    for exposure in (1.0, 0.37):
        check_pixels(enc, hdr, fbw, fbh, ss, exposure, ("drawn", exposure))
    specials = ppi.NONFINITE_SPECIALS + ppi.FINITE_SPECIALS
    for j, v in enumerate(specials * 2):
        y, x = (j * 7) % H, (j * 5) % W
        if j < len(specials):
            hdr[y, x, j % 3] = v
        else:
            hdr[y, x, :] = v
    check_pixels(enc, hdr, fbw, fbh, ss, 0.8, "specials")


def test_pixels_straddle_every_quantiser_step(enc):
    """inputs whose sRGB8 bytes lie on both sides of every step of both quantiser rules: for each byte a linear value found by bisection of
    the restatement itself (a grey pixel under exposure 1), every byte at every entry of the matrix"""
    lo, hi = np.zeros(256), np.full(256, 32.0)
    grey = lambda v: X.pixels(np.repeat(np.asarray(v, f32)[None, :, None], 3, axis=2).repeat(2, axis=0), len(v), 1, 1, 1.0)[0][0, :, 0].astype(int)
    want = np.arange(256)
    for _ in range(30):
        mid = (lo + hi) / 2
        got = grey(mid)
        hi = np.where(got >= want, mid, hi)
        lo = np.where(got < want, mid, lo)
    reached = grey(hi)
    assert len(set(reached.tolist())) >= 250, "the search reaches (nearly) every byte"
    steps = {(v + 25) // 51 for v in reached} | {(32 * v + 102 * d + 51) // 1632 for v in reached for d in range(16)}
    assert steps == set(range(6))
    # 4 x 256 x 4 pixels a half-cell row: each byte under all 16 matrix entries, in r, g and b separately
    fbw, fbh, ss = 256, 2, 4
    hdr = np.zeros((2 * fbh * ss, fbw * ss, 3), f32)
    for ch in range(3):
        hdr[4 * ch:4 * ch + 4, :, ch] = np.repeat(hi.astype(f32), 4)[None, :]
    hdr[12:16] = np.repeat(hi.astype(f32), 4)[None, :, None]
    wrgba = check_pixels(enc, hdr, fbw, fbh, ss, 1.0, "steps")
    assert len(np.unique(wrgba[12:16, :, 0])) >= 250


# ------------------------------------------------------------------------------------------------------------- 3: frames
FBW, FBH = 80, 45


@pytest.mark.parametrize("ss", [1, 2])
def test_frames_beside_a_twin(product_lib, ss):
    a, b, pose = S.twins(1, FBW, FBH, ss)
    try:
        registers = set()
        for k in range(3):
            S.move((a, b), pose, k)
            dither = k == 1
            if k < 2:
                plain = a.TryFlipAndBlitChexels(color16=False, rgba=True, sdr=True)
                out = b.TryFlipAndBlitPixels(rgba=True, index=True, dither=dither, sdr=True)
                stream = None
            else:
                plain = a.TryFlipAndBlitChexels(color16=False, rgba=True, sdr=True)
                stream, sdr = b.TryFlipAndBlitSixel((3, 2), clear_screen=True, dither=dither, sdr=True)
                out = {"sdr": sdr}
            assert pu.bits_equal(plain["sdr"], out["sdr"]), k
            assert a.stats.frame == b.stats.frame and a.stats.exposure == b.stats.exposure, k
            assert pu.bits_equal(a.read(abi.BUF_TAA_HISTORY), b.read(abi.BUF_TAA_HISTORY)), k
            wrgba, windex = X.pixels(b.read(abi.BUF_DENOISED), FBW, FBH, ss, b.stats.exposure, dither)
            if stream is None:
                assert np.array_equal(out["rgba"], wrgba) and np.array_equal(out["index"], windex), k
                if ss == 1:
                    assert np.array_equal(out["rgba"], plain["rgba"]), "at super_sample 1 the RGBA plane is the chexel call's"
            else:
                S.assert_stream(stream, X.encode(windex, (3, 2), True), k)
                plane, vp, clear, palette = X.decode(stream)
                assert np.array_equal(plane, windex) and vp == (3, 2) and clear and len(palette) == 216
            registers |= set(np.unique(windex).tolist())
        assert len(registers) >= 12          # (a picture, not one flat colour)
        # any subset of the destinations: the registers alone, the SDR alone
        S.move((a, b), pose, 3)
        plain = a.TryFlipAndBlit(want_sdr=True)
        only = b.TryFlipAndBlitPixels(rgba=False, index=True)
        assert list(only) == ["index"] and np.array_equal(only["index"], X.pixels(b.read(abi.BUF_DENOISED), FBW, FBH, ss, b.stats.exposure)[1])
        S.move((a, b), pose, 4)
        plain = a.TryFlipAndBlit(want_sdr=True)
        only = b.TryFlipAndBlitPixels(rgba=False, index=False, sdr=True)
        assert pu.bits_equal(plain, only["sdr"]) and a.stats.frame == b.stats.frame
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------- 4: state and refusals
CW, CH, VP = 84, 47, (2, 1)


@pytest.fixture()
def one(product_lib):
    a, b, pose = S.twins(1, FBW, FBH, 2)
    a.close()
    yield b
    b.close()


def test_a_sixel_frame_invalidates_the_delta_state_and_a_pixels_frame_does_not(one):
    g = one
    keyframe = lambda: g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)[1]["keyframe"]
    assert keyframe() == 1 and keyframe() == 0
    g.TryFlipAndBlitPixels()
    assert keyframe() == 0, "the planes call leaves the delta state alone"
    stream = g.TryFlipAndBlitSixel(VP)
    assert stream.startswith(b"\x1b[2;3H\x1bPq") and stream.endswith(b"\x1b\\")
    assert keyframe() == 1, "a delta behind a sixel frame is a keyframe"
    assert keyframe() == 0
    g.TryFlipAndBlitSixel(VP)
    assert g.TryFlipAndBlitAnsiDelta(CW, CH, VP, 3, 12)[1]["keyframe"] == 1 and g.TryFlipAndBlitAnsiQuadDelta(CW, CH, VP, 3, 12)[1]["keyframe"] == 1


def test_refusals_leave_the_context_and_the_delta_state(one):
    g = one
    L = g.L
    keyframe = lambda: g.TryFlipAndBlitAnsiRgbDelta(CW, CH, VP, 3, 12)[1]["keyframe"]
    assert keyframe() == 1
    frame0 = g.stats.frame
    history = g.read(abi.BUF_TAA_HISTORY).copy()
    W, H = FBW * 2, FBH * 4
    cap = RaytraceRenderer.sixel_stream_bound(W, H, L)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    index = np.zeros((H, W), np.uint8)
    p, ip = out.ctypes.data_as(U8P), index.ctypes.data_as(U8P)
    sixel = lambda vx=0, vy=0, dither=0, o=p, c=cap, ln=C.byref(n): L.ycge_render_frame_sixel(g.ctx, vx, vy, 0, dither, o, c, ln, None, None)
    planes = lambda dither=0, i=ip: L.ycge_render_frame_pixels(g.ctx, None, None, i, dither, None)
    for call, words in [(lambda: sixel(o=None), [b"NULL"]), (lambda: sixel(ln=None), [b"NULL"]), (lambda: sixel(c=cap - 1), [b"capacity %d" % (cap - 1)]),
                        (lambda: sixel(vx=-1), [b"(-1, 0)"]), (lambda: sixel(vy=-7), [b"(0, -7)"]), (lambda: sixel(dither=2), [b"dither 2"]),
                        (lambda: sixel(dither=-1), [b"dither -1"]), (lambda: planes(2), [b"dither 2"]), (lambda: planes(0, None), [b"every destination is NULL"])]:
        rc = call()
        msg = L.ycge_last_error(g.ctx)
        assert rc == abi.YCGE_ERR_INVALID_ARG and all(w in msg for w in words), msg
    assert not out.any() and n.value == 0 and not index.any()
    assert pu.bits_equal(g.read(abi.BUF_TAA_HISTORY), history)
    assert keyframe() == 0, "a refused call forces no keyframe"
    assert g.stats.frame == frame0 + 1


def test_a_peer_context_is_refused(product_lib):
    a, b, pose = S.twins(2, 160, 45, 2, devices=[0, 0, 0])
    try:
        a.close()
        fn = b.L.ycge_debug_peer_context
        fn.restype, fn.argtypes = abi.HOOK_PROTOTYPES["ycge_debug_peer_context"]
        peer = fn(b.ctx, 0)
        assert peer
        index = np.zeros((180, 320), np.uint8)
        assert b.L.ycge_render_frame_pixels(peer, None, None, index.ctypes.data_as(U8P), 0, None) == abi.YCGE_ERR_INVALID_ARG
        cap = RaytraceRenderer.sixel_stream_bound(320, 180, b.L)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        assert b.L.ycge_render_frame_sixel(peer, 0, 0, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), None, None) == abi.YCGE_ERR_INVALID_ARG
        assert not index.any() and not out.any() and n.value == 0
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------------------- 5: the host fallback
CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import sixel_planes as P
import test_gpu_ansi_stream as S
import test_gpu_sixel as T
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
a, b, pose = S.twins(1, 16, 8, 2)
a.close()
plane = P.drawn(65, 13)[1]
out = dict(hook=T.hook_stream(b, plane, (9, 99), True).hex(), frame=b.TryFlipAndBlitSixel((1, 2), dither=True).hex())
b.close()
print("RESULT " + json.dumps(out))
"""


def test_the_host_fallback_gives_the_same_bytes(product_lib):
    a, b, pose = S.twins(1, 16, 8, 2)
    try:
        a.close()
        plane = P.drawn(65, 13)[1]
        want = dict(hook=hook_stream(b, plane, (9, 99), True).hex(), frame=b.TryFlipAndBlitSixel((1, 2), dither=True).hex())
    finally:
        b.close()
    assert bytes.fromhex(want["hook"]) == X.encode(plane, (9, 99), True)
    env = dict(os.environ, YCGE_SIXEL_HOST="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(tests=str(ROOT / "tests"), root=str(ROOT))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    assert got == want
