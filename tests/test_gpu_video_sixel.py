"""Sixel in Video mode on the GPU: k_video_pixels alone through ycge_test_video_pixels against tests/sixel_delta_restatement.video_pixels,
byte for byte; ycge_video_blit_pixels beside ycge_video_blit; ycge_video_blit_sixel against the restatement's stream of the plane;
ycge_video_blit_sixel_delta on a still and on a changing source, and the delta state it shares with the frame calls.  Every comparison
is exact."""
import ctypes as C

import numpy as np
import pytest

import parity_util as pu
import sixel_delta_restatement as D
import sixel_planes as P
import sixel_restatement as X
import test_gpu_ansi_stream as S
import video_quadrant_inputs as I
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VideoRenderer

pytestmark = pytest.mark.gpu
U8P = C.POINTER(C.c_uint8)
EXPORTS = ("ycge_video_blit_pixels", "ycge_video_blit_sixel", "ycge_video_blit_sixel_delta", "ycge_test_video_pixels")
# (src_w, src_h, fbW, fbH, ss): upscale with every tap clamped; 66 columns, a second wavefront; letterbox top and bottom; letterbox left and
# right; the smallest case
HOOK_CASES = [(3, 2, 5, 2, 3), (64, 48, 33, 3, 2), (200, 40, 7, 5, 1), (40, 200, 16, 4, 4), (1, 1, 1, 1, 1)]


@pytest.fixture(scope="module")
def lib(product_lib):
    """the exports, looked up first: a library without them fails here, it does not skip"""
    for n in EXPORTS:
        assert getattr(product_lib, n) is not None
    return product_lib


@pytest.fixture(scope="module")
def vid(lib):
    v = VideoRenderer(20, 5, 2, lib=lib)          # no scene, ever
    yield v
    v.close()


# ------------------------------------------------------------------------------------------------------------- 1: the kernel alone
@pytest.mark.parametrize("case", HOOK_CASES, ids=lambda c: "%dx%d-%dx%d-ss%d" % c)
@pytest.mark.parametrize("bpp", [3, 4])
def test_kernel_equals_the_restatement(vid, case, bpp):
    sw, sh, fw, fh, ss = case
    frames = [("noise", I.noise(sw, sh, bpp)), ("all 255", I.constant(sw, sh, bpp, 255)), ("all 0", I.constant(sw, sh, bpp, 0))]
    if sw > 8 and sh > 8:
        frames.append(("drawn", I.drawn(sw, sh, bpp)))
    for kind, f in frames:
        for dither in (0, 1):
            rgba, index = vid.pixels_probe(f, fw, fh, ss, dither)
            wrgba, windex = D.video_pixels(f, sw, sh, bpp, fw, fh, ss, dither)
            assert np.array_equal(rgba, wrgba), (case, bpp, kind, dither, np.argwhere(rgba != wrgba)[:4])
            assert np.array_equal(index, windex), (case, bpp, kind, dither, np.argwhere(index != windex)[:4])
        if kind == "all 0":
            assert not rgba[..., :3].any() and not index.any()


def test_hook_refusals(vid):
    fn = vid.L.ycge_test_video_pixels
    fn.restype, fn.argtypes = abi.SIXEL_DELTA_HOOK_PROTOTYPES["ycge_test_video_pixels"]
    f = I.noise(7, 5, 3)
    rgba, index = np.full((4, 3, 4), 7, np.uint8), np.full((4, 3), 7, np.uint8)
    p = f.ctypes.data_as(U8P)
    for args in [(None, 7, 5, 3, 3, 2, 1, 0, rgba.ctypes.data, index.ctypes.data), (p, 7, 5, 3, 3, 2, 1, 0, None, None), (p, 7, 5, 2, 3, 2, 1, 0, rgba.ctypes.data, None),
                 (p, 0, 5, 3, 3, 2, 1, 0, rgba.ctypes.data, None), (p, 7, 5, 3, 3, 2, 0, 0, rgba.ctypes.data, None), (p, 7, 5, 3, 3, 2, 1, 2, rgba.ctypes.data, None)]:
        assert fn(vid.ctx, *args) == abi.YCGE_ERR_INVALID_ARG
    assert (rgba == 7).all() and (index == 7).all()
    assert fn(vid.ctx, p, 7, 5, 3, 3, 2, 1, 0, rgba.ctypes.data, None) == 0 and (rgba[..., 3] == 255).all() and (index == 7).all()


# ------------------------------------------------------------------------------------------------------------- 2: the exports
@pytest.mark.parametrize("ss", [1, 2])
def test_planes_beside_the_blit(lib, ss):
    sw, sh, bpp, fw, fh = 40, 30, 4, 20, 5
    f = I.drawn(sw, sh, bpp)
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        plain = v.TryFlipAndBlit(f, color16=False, rgba=True, sdr=True)
        for dither in (False, True):
            out = v.TryFlipAndBlitPixels(f, dither=dither, sdr=True)
            assert pu.bits_equal(out["sdr"], plain["sdr"]), "the SDR is ycge_video_blit's, bit for bit"
            wrgba, windex = D.video_pixels(f, sw, sh, bpp, fw, fh, ss, int(dither))
            assert np.array_equal(out["rgba"], wrgba) and np.array_equal(out["index"], windex), (ss, dither)
            if ss == 1:
                assert np.array_equal(out["rgba"], plain["rgba"]), "at super_sample 1 the RGBA plane is ycge_video_blit's"
        only = v.TryFlipAndBlitPixels(f, rgba=False, index=True)
        assert list(only) == ["index"] and np.array_equal(only["index"], D.video_pixels(f, sw, sh, bpp, fw, fh, ss)[1])
        only = v.TryFlipAndBlitPixels(f, rgba=False, index=False, sdr=True)
        assert pu.bits_equal(only["sdr"], plain["sdr"])


def sixel_call(v, f, delta, vp=(2, 1), clear=0, keyframe=0, dither=0):
    """the stream call into a buffer of the bound's size with a canary behind it: (bytes, info or None)"""
    W, H = v.fbW * v.ss, 2 * v.fbH * v.ss
    cap = X.bound(W, H)
    out, n, info = np.full(cap + 64, P.CANARY, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    p, o = f.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
    if delta:
        rc = v.L.ycge_video_blit_sixel_delta(v.ctx, p, f.shape[1], f.shape[0], f.shape[2], vp[0], vp[1], clear, keyframe, dither, o, cap, C.byref(n), info, None)
    else:
        rc = v.L.ycge_video_blit_sixel(v.ctx, p, f.shape[1], f.shape[0], f.shape[2], vp[0], vp[1], clear, dither, o, cap, C.byref(n), None)
    v._r._check(rc)
    assert n.value <= cap and (out[n.value:] == P.CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), tuple(info) if delta else None


@pytest.mark.parametrize("sw,sh,bpp,fw,fh,ss", [(16, 12, 3, 65, 9, 2), (40, 30, 4, 20, 5, 4)])
def test_stream_is_the_encoding_of_the_plane(lib, sw, sh, bpp, fw, fh, ss):
    f = I.drawn(sw, sh, bpp)
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        for dither, clear in ((0, 1), (1, 0)):
            windex = D.video_pixels(f, sw, sh, bpp, fw, fh, ss, dither)[1]
            got, _ = sixel_call(v, f, False, (3, 2), clear, dither=dither)
            S.assert_stream(got, X.encode(windex, (3, 2), bool(clear)), (dither, clear))
        stream, sdr = v.TryFlipAndBlitSixel(f, (3, 2), sdr=True)
        assert pu.bits_equal(sdr, v.TryFlipAndBlit(f, color16=False, sdr=True)["sdr"]) and np.array_equal(X.decode(stream)[0], D.video_pixels(f, sw, sh, bpp, fw, fh, ss)[1])


def test_delta_of_a_still_and_of_a_changing_source(lib):
    sw, sh, bpp, fw, fh, ss = 40, 30, 4, 20, 5, 4
    a, _, b, _ = I.sequence(sw, sh, bpp)
    W, H = fw * ss, 2 * fh * ss
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        pa, pb = (D.video_pixels(f, sw, sh, bpp, fw, fh, ss, 1)[1] for f in (a, b))
        got, info = sixel_call(v, a, True, dither=1)
        assert info == (1, 0, 0, 0)
        S.assert_stream(got, X.encode(pa, (2, 1)), "the first call is _sixel's stream")
        got, info = sixel_call(v, a.copy(), True, dither=1)
        assert info == (0, 0, 0, 0) and got == D.delta_header(W, H, (2, 1)) + b"\x1b\\", "a still source: header and trailer"
        got, info = sixel_call(v, b, True, dither=1)
        want, winfo = D.encode_delta(pa, pb, (2, 1))
        S.assert_stream(got, want, "one block changed")
        assert info == winfo and 0 < info[1] < -(-H // 6) and info[2] < W * H // 2
        screen, painted = D.apply(got, pa, pb)
        assert np.array_equal(screen, pb)
        # the painted pixels lie in the bands and columns that cover the block's reach: the rows and columns in which the planes differ
        ys, xs = np.nonzero(pa != pb)
        py, px = np.nonzero(painted)
        assert py.min() // 6 == ys.min() // 6 and py.max() // 6 == ys.max() // 6 and px.min() >= xs.min() and px.max() <= xs.max()
        got, info = sixel_call(v, a, True, dither=1)
        S.assert_stream(got, D.encode_delta(pb, pa, (2, 1))[0], "and back")


def test_state_is_shared_with_the_frames(lib):
    FBW, FBH, SS, VP = 40, 12, 2, (2, 1)
    a, g, pose = S.twins(1, FBW, FBH, SS)
    a.close()
    try:
        v = VideoRenderer(renderer=g)
        f = I.drawn(40, 30, 3)
        frame_key = lambda **kw: g.TryFlipAndBlitSixelDelta(VP, **kw)[1][0]
        video = lambda **kw: v.TryFlipAndBlitSixelDelta(f, VP, **kw)
        assert frame_key() == 1 and frame_key() == 0
        shown = g.TryFlipAndBlitSixelDelta(VP, keyframe=True)[0]
        stream, info = video()
        assert info[0] == 0, "a frame delta then a video delta on one geometry is a delta"
        want = D.video_pixels(f, 40, 30, 3, FBW, FBH, SS)[1]
        assert np.array_equal(D.apply(stream, X.decode(shown)[0], want)[0], want), "the film painted over the traced picture"
        stream, info = video()
        assert info == (0, 0, 0, 0)
        assert frame_key() == 0, "and back to frames"
        assert video(keyframe=True)[1][0] == 1 and video()[1][0] == 0
        assert video(clear_screen=True)[1][0] == 1 and video()[1][0] == 0
        assert v.TryFlipAndBlitSixelDelta(f, (3, 1))[1][0] == 1 and video()[1][0] == 1 and video()[1][0] == 0
        v.TryFlipAndBlitPixels(f)
        assert video()[1][0] == 0, "the planes call leaves the state alone"
        v.TryFlipAndBlitSixel(f, VP)
        assert video()[1][0] == 1 and video()[1][0] == 0, "a plain _sixel call"
        assert v.TryFlipAndBlitAnsiRgbDelta(f, 44, 14, VP, 3, 12)[1]["keyframe"] == 1
        assert video()[1][0] == 1 and video()[1][0] == 0, "an _ansi_rgb_delta call"
        assert v.TryFlipAndBlitAnsiRgbDelta(f, 44, 14, VP, 3, 12)[1]["keyframe"] == 1, "an ANSI delta after a sixel delta is a keyframe"
        assert video()[1][0] == 1
        # a refused call leaves the next call a delta
        cap = X.bound(FBW * SS, 2 * FBH * SS)
        out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
        p, o = f.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
        L = v.L
        for rc in (L.ycge_video_blit_sixel_delta(v.ctx, p, 40, 30, 3, -1, 0, 0, 0, 0, o, cap, C.byref(n), None, None),
                   L.ycge_video_blit_sixel_delta(v.ctx, p, 40, 30, 3, 2, 1, 0, 0, 0, o, cap - 1, C.byref(n), None, None),
                   L.ycge_video_blit_sixel_delta(v.ctx, p, 40, 30, 2, 2, 1, 0, 0, 0, o, cap, C.byref(n), None, None),
                   L.ycge_video_blit_sixel_delta(v.ctx, None, 40, 30, 3, 2, 1, 0, 0, 0, o, cap, C.byref(n), None, None),
                   L.ycge_video_blit_sixel_delta(v.ctx, p, 40, 30, 3, 2, 1, 0, 0, 2, o, cap, C.byref(n), None, None),
                   L.ycge_video_blit_sixel(v.ctx, p, 40, 30, 3, 2, 1, 0, 0, None, cap, C.byref(n), None),
                   L.ycge_video_blit_pixels(v.ctx, p, 40, 30, 3, None, None, None, 0)):
            assert rc == abi.YCGE_ERR_INVALID_ARG
        assert not out.any() and n.value == 0
        assert video()[1][0] == 0, "a refused call forces no keyframe"
        g.Resize(FBW, FBH, SS)
        assert video()[1][0] == 1 and video()[1][0] == 0, "ycge_resize"
    finally:
        g.close()
