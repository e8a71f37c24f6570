"""Quadrant glyphs in Video mode on the GPU: k_video_blit_quadrants alone through its hook, ycge_video_blit_quadrants / _ansi_quad /
_ansi_quad_delta on a context, the delta state shared with the frame quad streams, and the refusals - against
tests/video_quadrant_restatement.py for the colours and tests/quadrant_restatement.py for the planes and the streams.  Every comparison is
bit for bit: float arrays through their uint32 view, streams as bytes.  What the inputs reach (every mask, flat cells, clamped taps, the
last 3-byte pixel, halves that do not add up to the serial sum) is asserted without a GPU in tests/test_video_quadrants_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import ansi_layers_restatement as LR
import parity_util as pu
import quadrant_restatement as Q
import test_gpu_ansi_stream as S
import video_quadrant_inputs as I
import video_quadrant_restatement as VQ
import video_restatement as VR
from yetanotherconsolegameengine_amd import abi
from yetanotherconsolegameengine_amd.renderer import ConsoleLayer, RaytraceRenderer, VideoRenderer

pytestmark = pytest.mark.gpu
f32 = np.float32
U8P, U16P, F32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_float)
CANARY = S.CANARY
EXPORTS = ("ycge_video_blit_quadrants", "ycge_video_blit_ansi_quad", "ycge_video_blit_ansi_quad_delta", "ycge_test_video_blit_quadrants")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"


@pytest.fixture(scope="module")
def lib(product_lib):
    """the exports, looked up first: a library without them fails here, it does not skip"""
    for n in EXPORTS:
        assert getattr(product_lib, n) is not None
    return product_lib


@pytest.fixture(scope="module")
def vid(lib):
    v = VideoRenderer(8, 4, 2, lib=lib)          # no scene, ever
    yield v
    v.close()


_wanted = {}


def wanted(case):
    """case -> what the restatement gives for its sequence's frames 0 and 2, computed once and left unchanged: a list of dicts with the frame,
    sdr, quad_sdr and per min_contrast the planes"""
    if case not in _wanted:
        sw, sh, bpp, fw, fh, ss = case
        seq = I.sequence(sw, sh, bpp)
        out = []
        for f in (seq[0], seq[2]):
            sdr, quad = VQ.blit_quadrants(f, sw, sh, bpp, fw, fh, ss)
            out.append({"frame": f, "sdr": sdr, "quad_sdr": quad, "planes": {mc: Q.planes(quad, fw, fh, mc) for mc in (0, 8)}})
        _wanted[case] = out
    return _wanted[case]


# ------------------------------------------------------------------------------------------------------------- 1: the kernel alone
@pytest.mark.parametrize("case", I.HOOK_CASES, ids=I.case_id)
def test_kernel_equals_the_restatement(vid, case):
    sw, sh, bpp, fw, fh, ss = case
    for kind, f in (("noise", I.noise(sw, sh, bpp)), ("all 255", I.constant(sw, sh, bpp, 255)), ("all 0", I.constant(sw, sh, bpp, 0))):
        sdr, quad = vid.blit_quadrants_probe(f, fw, fh, ss)
        w_sdr, w_quad = VQ.blit_quadrants(f, sw, sh, bpp, fw, fh, ss)
        assert_bits(sdr, w_sdr, f"{case} {kind} sdr")
        assert_bits(quad, w_quad, f"{case} {kind} quad_sdr")
        assert not np.isnan(quad).any()
        if kind == "all 0":
            assert not bits(sdr).any() and not bits(quad).any()
        if kind == "all 255" and case in I.ONES_EXACT_CASES:
            assert (sdr == 1).all() and (quad == 1).all()
    # the serial sum is k_video_blit's own
    f = I.noise(sw, sh, bpp)
    assert_bits(vid.blit_quadrants_probe(f, fw, fh, ss)[0], vid.blit_probe(f, fw, fh, ss), f"{case} against k_video_blit")


def test_kernel_equals_the_scalar_form(vid):
    """the literal per-sample form against the kernel directly (small: it is a Python loop)"""
    f = I.noise(7, 6, 3, 9)
    sdr, quad = vid.blit_quadrants_probe(f, 5, 3, 2)
    w_sdr, w_quad = VQ.blit_quadrants_scalar(f, 7, 6, 3, 5, 3, 2)
    assert_bits(sdr, w_sdr, "sdr"); assert_bits(quad, w_quad, "quad_sdr")


def test_hook_refusals(vid):
    fn = vid.L.ycge_test_video_blit_quadrants
    fn.restype, fn.argtypes = abi.VIDEO_HOOK_PROTOTYPES["ycge_test_video_blit_quadrants"]
    f = I.noise(7, 5, 3)
    sdr, quad = np.full((2, 3, 2, 3), 7.0, f32), np.full((2, 3, 4, 3), 7.0, f32)
    for ss in (1, 3, 0):
        assert fn(vid.ctx, f.ctypes.data, 7, 5, 3, 3, 2, ss, sdr.ctypes.data, quad.ctypes.data) == abi.YCGE_ERR_INVALID_ARG
        assert b"%d" % ss in vid.L.ycge_last_error(vid.ctx)
    assert fn(vid.ctx, None, 7, 5, 3, 3, 2, 2, sdr.ctypes.data, quad.ctypes.data) == abi.YCGE_ERR_INVALID_ARG
    assert fn(vid.ctx, f.ctypes.data, 7, 5, 3, 3, 2, 2, sdr.ctypes.data, None) == abi.YCGE_ERR_INVALID_ARG
    assert (sdr == 7).all() and (quad == 7).all()
    assert fn(vid.ctx, f.ctypes.data, 7, 5, 3, 3, 2, 2, sdr.ctypes.data, quad.ctypes.data) == 0 and (quad != 7).all()


# ------------------------------------------------------------------------------------------------------------- 2: the planes call on a context
def quad_shapes(fw, fh):
    return {"sdr": ((fh, fw, 2, 3), np.float32), "quad_sdr": ((fh, fw, 4, 3), np.float32), "glyphs": ((fh, fw), np.uint16), "rgba": ((2 * fh, fw, 4), np.uint8)}


def assert_planes(got, want, mc, what):
    for k, a in got.items():
        if k in ("sdr", "quad_sdr"):
            assert_bits(a, want[k], f"{what} {k}")
        else:
            w = want["planes"][mc][0 if k == "glyphs" else 1]
            assert a.shape == w.shape and np.array_equal(a, w), f"{what} {k}: {np.count_nonzero(a != w)} differ"


@pytest.mark.parametrize("case", I.CONTEXT_CASES, ids=I.case_id)
def test_planes_of_a_context(lib, case):
    sw, sh, bpp, fw, fh, ss = case
    want = wanted(case)
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        seen = set()
        for k, w in enumerate(want):
            for mc in (0, 8):
                got = v.TryFlipAndBlitQuadrants(w["frame"], quad_sdr=True, glyphs=True, rgba=True, sdr=True, min_contrast=mc)
                assert sorted(got) == ["glyphs", "quad_sdr", "rgba", "sdr"]
                assert_planes(got, w, mc, f"frame {k} min_contrast {mc}")
                seen |= set(got["glyphs"].ravel().tolist())
            assert_bits(v.TryFlipAndBlit(w["frame"], color16=False, sdr=True)["sdr"], w["sdr"], "ycge_video_blit's sdr on the same context")
        assert seen == set(Q.GLYPHS)
        # any subset of the destinations
        w = want[0]
        for names in (("sdr",), ("quad_sdr",), ("glyphs",), ("rgba",), ("glyphs", "rgba"), ("sdr", "glyphs"), ("quad_sdr", "rgba")):
            got = v.TryFlipAndBlitQuadrants(w["frame"], **{k: k in names for k in ("sdr", "quad_sdr", "glyphs", "rgba")}, min_contrast=8)
            assert sorted(got) == sorted(names)
            assert_planes(got, w, 8, f"{names} alone")


def test_planes_pageable_and_page_locked(lib):
    case = I.CONTEXT_CASES[0]
    sw, sh, bpp, fw, fh, ss = case
    w = wanted(case)[1]
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        r = v._r
        for frame_locked in (False, True):
            for dst_locked in (False, True):
                f = w["frame"]
                if frame_locked:
                    f = r._page_locked_zeros(w["frame"].shape, np.uint8)[0]
                    f[...] = w["frame"]
                out = {k: (r._page_locked_zeros(shp, dt)[0] if dst_locked else np.zeros(shp, dt)) for k, (shp, dt) in quad_shapes(fw, fh).items()}
                if dst_locked:
                    assert all(v.L.ycge_debug_is_page_locked(a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)) == 1 for a in out.values())
                assert_planes(v.TryFlipAndBlitQuadrants(f, out=out, min_contrast=8), w, 8, f"frame locked {frame_locked}, destinations locked {dst_locked}")


# ------------------------------------------------------------------------------------------------------------- 3: the streams
def console_of(fw, fh):
    return fw + 3, fh + 2, (2, 1)


@pytest.mark.parametrize("case", I.CONTEXT_CASES, ids=I.case_id)
def test_full_stream(lib, case):
    sw, sh, bpp, fw, fh, ss = case
    w = wanted(case)[0]
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        for mc in (0, 8):
            glyphs, rgba = w["planes"][mc]
            for cw, ch, vp, clear in ((fw, fh, (0, 0), False), console_of(fw, fh) + (False,), console_of(fw, fh) + (True,), (fw + 1, fh, (-1, 0), True)):
                got, sdr = v.TryFlipAndBlitAnsiQuad(w["frame"], cw, ch, vp, 3, 12, clear_screen=clear, min_contrast=mc, sdr=True)
                S.assert_stream(got, Q.stream(glyphs, rgba, cw, ch, vp, 3, 12, clear=clear), (cw, ch, vp, clear, mc))
                assert_bits(sdr, w["sdr"], "stream form sdr")
        # its exact length, never a byte past it: a pageable buffer with a canary behind the bound
        cw, ch, vp = console_of(fw, fh)
        cap = RaytraceRenderer.ansi_rgb_stream_bound(cw, ch, v.L)
        out, n = np.full(cap + 64, CANARY, np.uint8), C.c_size_t(0)
        f = w["frame"]
        v._r._check(v.L.ycge_video_blit_ansi_quad(v.ctx, f.ctypes.data_as(U8P), sw, sh, bpp, cw, ch, vp[0], vp[1], 3, 12, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), None))
        glyphs, rgba = w["planes"][0]
        assert out[:n.value].tobytes() == Q.stream(glyphs, rgba, cw, ch, vp, 3, 12) and (out[n.value:] == CANARY).all()


def menu(x, y):
    """a 6 x 2 framebuffer above the raytrace one"""
    chars = np.full((2, 6), ord("+"), np.uint16)
    chars[0, 1:5] = [ord(ch) for ch in "menu"]
    chars[1, 2] = 0x20
    return [LR.Layer(chars, (1.0, 1.0, 0.0), (0.5, 0.5, 0.5), x, y)]


def mirror(layers):
    return [ConsoleLayer(l.chars, l.fg, l.bg, l.x, l.y) for l in layers]


@pytest.mark.parametrize("tol", [0, 2])
@pytest.mark.parametrize("case", I.CONTEXT_CASES, ids=I.case_id)
def test_delta_sequence_of_four_frames(lib, case, tol):
    """a keyframe, the same frame again, a changed region, then the same picture under a layer that moved"""
    sw, sh, bpp, fw, fh, ss = case
    want = wanted(case)
    seq = I.sequence(sw, sh, bpp)
    cw, ch, vp = console_of(fw, fh)
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        shown = None
        for k, f in enumerate(seq):
            layers = menu(4 if k < 3 else 7, 1 if k < 3 else 2)
            v.SetConsoleLayers(mirror(layers), 0)
            w = want[0 if k < 2 else 1]
            assert np.array_equal(f, w["frame"])
            stream, info, sdr = v.TryFlipAndBlitAnsiQuadDelta(f, cw, ch, vp, 3, 12, merge_gap=2, tolerance=tol, sdr=True)
            glyphs, rgba = w["planes"][0]
            wstream, winfo, shown = Q.delta(shown, glyphs, rgba, cw, ch, vp, 3, 12, gap=2, tol=tol, layers=layers, raytrace_at=0)
            S.assert_stream(stream, wstream, ("delta", k))
            assert info == winfo and info["keyframe"] == int(k == 0), (k, info, winfo)
            assert_bits(sdr, w["sdr"], f"delta form sdr {k}")
            if k == 0:
                S.assert_stream(stream, Q.stream(glyphs, rgba, cw, ch, vp, 3, 12, layers=layers, raytrace_at=0), "the keyframe is the full stream")
            if k == 1:
                assert info == dict(keyframe=0, changed=0, emitted=1, runs=1)          # only the last cell is emitted
            if k >= 2:
                assert 0 < info["changed"] < cw * ch


# ------------------------------------------------------------------------------------------------------------- 4: state
FW, FH, SS = I.CONTEXT_CASES[0][3:]
CW, CH, VP = console_of(FW, FH)


def frame_planes(g, mc=0):
    quad = Q.sub_cells(g.read(abi.BUF_DENOISED), g.fbW, g.fbH, g.ss, g.stats.exposure)
    return Q.planes(quad, g.fbW, g.fbH, mc)


def video_step(v, w, shown, keyframe_expected, what, mc=0, tol=0):
    """one video _quad_delta of v held to the restatement against `shown`; -> the next shown"""
    stream, info = v.TryFlipAndBlitAnsiQuadDelta(w["frame"], CW, CH, VP, 3, 12, merge_gap=2, tolerance=tol, min_contrast=mc)
    glyphs, rgba = w["planes"][mc]
    want, winfo, nxt = Q.delta(None if keyframe_expected else shown, glyphs, rgba, CW, CH, VP, 3, 12, gap=2, tol=tol)
    S.assert_stream(stream, want, what)
    assert info == winfo and info["keyframe"] == int(keyframe_expected), (what, info, winfo)
    return nxt


def frame_step(g, shown, keyframe_expected, what):
    stream, info = g.TryFlipAndBlitAnsiQuadDelta(CW, CH, VP, 3, 12, merge_gap=2)
    glyphs, rgba = frame_planes(g)
    want, winfo, nxt = Q.delta(None if keyframe_expected else shown, glyphs, rgba, CW, CH, VP, 3, 12, gap=2)
    S.assert_stream(stream, want, what)
    assert info == winfo and info["keyframe"] == int(keyframe_expected), (what, info, winfo)
    return nxt


@pytest.fixture()
def both(lib):
    """the mode switch of RaytraceEntity: both renderers of one console on one context (the small Cornell scene), and a twin that never blits"""
    a, b, pose = S.twins(1, FW, FH, SS)
    yield a, b, VideoRenderer(renderer=b), pose
    a.close(); b.close()


def test_the_video_and_frame_quad_streams_share_one_delta_state(both):
    a, g, v, pose = both
    w0, w1 = wanted(I.CONTEXT_CASES[0])
    s = video_step(v, w0, None, True, "first")
    s = video_step(v, w0, s, False, "a video delta")
    s = video_step(v, w1, s, False, "min_contrast is no part of the key", mc=8)
    s = frame_step(g, s, False, "a frame delta behind a video delta of the same key")
    s = video_step(v, w1, s, False, "a video delta behind a frame delta of the same key")
    v.TryFlipAndBlitAnsiRgb(w0["frame"], CW, CH, VP, 3, 12)
    s = video_step(v, w0, s, True, "a video quad delta behind ycge_video_blit_ansi_rgb")
    _, info = v.TryFlipAndBlitAnsiRgbDelta(w0["frame"], CW, CH, VP, 3, 12)
    assert info["keyframe"] == 1, "a 24-bit delta behind a video quad delta"
    s = video_step(v, w0, s, True, "a video quad delta behind a 24-bit delta")
    v.TryFlipAndBlitAnsiQuad(w0["frame"], CW, CH, VP, 3, 12)
    s = video_step(v, w0, s, True, "behind a full video quad stream")
    # blits that hand out no stream leave the state alone
    v.TryFlipAndBlitQuadrants(w1["frame"])
    v.TryFlipAndBlit(w1["frame"])
    s = video_step(v, w1, s, False, "behind ycge_video_blit_quadrants and ycge_video_blit")
    stream, info = v.TryFlipAndBlitAnsiQuadDelta(w1["frame"], CW + 1, CH, VP, 3, 12, merge_gap=2)
    assert info["keyframe"] == 1, "another console width"


def test_nothing_a_traced_frame_reads_moves(both):
    """frame / frame / quad blits / frame equals the twin's three frames; and ycge_video_blit after quad calls is what it was"""
    a, g, v, pose = both
    w0, w1 = wanted(I.CONTEXT_CASES[0])
    plain_before = v.TryFlipAndBlit(w0["frame"], color16=True, ansi=True, rgba=True, sdr=True)
    for k in range(3):
        S.move((a, g), pose, k)
        if k == 2:
            v.TryFlipAndBlitQuadrants(w0["frame"], quad_sdr=True, sdr=True, min_contrast=8)
            v.TryFlipAndBlitAnsiQuad(w1["frame"], CW, CH, VP, 3, 12)
            v.TryFlipAndBlitAnsiQuadDelta(w1["frame"], CW, CH, VP, 3, 12)
        sa, sb = a.TryFlipAndBlit(want_sdr=True), g.TryFlipAndBlit(want_sdr=True)
        assert pu.bits_equal(sa, sb), k
        assert a.stats.frame == g.stats.frame and a.stats.exposure == g.stats.exposure, k
    for which in (abi.BUF_TAA_HISTORY, abi.BUF_DENOISED, abi.BUF_PREV_DEPTH):
        assert a.read(which).tobytes() == g.read(which).tobytes(), which
    # the frame's own quadrant planes still come from the traced frame, not from the blit's sub-cell colours
    out = g.TryFlipAndBlitQuadrants(glyphs=True, rgba=True)
    glyphs, rgba = frame_planes(g)
    assert np.array_equal(out["glyphs"], glyphs) and np.array_equal(out["rgba"], rgba)
    plain_after = v.TryFlipAndBlit(w0["frame"], color16=True, ansi=True, rgba=True, sdr=True)
    for k in plain_before:
        assert plain_before[k].tobytes() == plain_after[k].tobytes(), k
    assert_bits(plain_after["sdr"], VR.blit(w0["frame"], *I.CONTEXT_CASES[0][:3], FW, FH, SS), "ycge_video_blit after quad calls")


def test_a_quad_blit_joins_the_frames_in_flight(both):
    a, g, v, pose = both
    w0 = wanted(I.CONTEXT_CASES[0])[0]
    g.RenderAsync()
    assert g.flight_info()["frames_outstanding"] == 1
    assert_planes(v.TryFlipAndBlitQuadrants(w0["frame"], quad_sdr=True, sdr=True), w0, 0, "blit behind a frame in flight")
    assert g.flight_info()["frames_outstanding"] == 0


# ------------------------------------------------------------------------------------------------------------- 5: refusals
def test_refusals_write_nothing_and_leave_the_state(lib):
    case = I.CONTEXT_CASES[0]
    sw, sh, bpp, fw, fh, ss = case
    w0, w1 = wanted(case)
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        L = v.L
        s = video_step(v, w0, None, True, "first")
        f = w0["frame"]
        fp = f.ctypes.data_as(U8P)
        cap = RaytraceRenderer.ansi_rgb_stream_bound(CW, CH, L)
        out, n, info = np.full(cap, CANARY, np.uint8), C.c_size_t(12345), (C.c_uint32 * 4)(9, 9, 9, 9)
        p = out.ctypes.data_as(U8P)
        arrs = {k: np.full(shp, CANARY if dt != np.float32 else 7.0, dt) for k, (shp, dt) in quad_shapes(fw, fh).items()}
        ptrs = lambda names=("sdr", "quad_sdr", "glyphs", "rgba"): [arrs[k].ctypes.data_as(t) if k in names else None
                                                                    for k, t in (("sdr", F32P), ("quad_sdr", F32P), ("glyphs", U16P), ("rgba", U8P))]
        planes = lambda mc=0, fr=fp, names=("sdr", "quad_sdr", "glyphs", "rgba"), w_=sw, bpp_=bpp: L.ycge_video_blit_quadrants(v.ctx, fr, w_, sh, bpp_, *ptrs(names), mc)
        full = lambda mc=0, c=cap, fr=fp, fg=3, o=p, ln=C.byref(n): L.ycge_video_blit_ansi_quad(v.ctx, fr, sw, sh, bpp, CW, CH, VP[0], VP[1], fg, 12, 0, mc, o, c, ln,
                                                                                                 arrs["sdr"].ctypes.data_as(F32P))
        delta = lambda mc=0, c=cap, fr=fp, gap=2, tol=0: L.ycge_video_blit_ansi_quad_delta(v.ctx, fr, sw, sh, bpp, CW, CH, VP[0], VP[1], 3, 12, 0, gap, tol, 0, mc, p, c,
                                                                                           C.byref(n), info, arrs["sdr"].ctypes.data_as(F32P))
        for call, words in [(lambda: planes(-1), [b"min_contrast -1"]), (lambda: planes(256), [b"min_contrast 256"]), (lambda: full(-1), [b"min_contrast -1"]),
                            (lambda: full(256), [b"min_contrast 256"]), (lambda: delta(-1), [b"min_contrast -1"]), (lambda: delta(256), [b"min_contrast 256"]),
                            (lambda: planes(0, fp, ()), [b"every destination is NULL"]), (lambda: planes(0, None), [b"frame is NULL"]),
                            (lambda: full(0, cap, None), [b"frame is NULL"]), (lambda: delta(0, cap, None), [b"frame is NULL"]),
                            (lambda: planes(0, fp, ("glyphs",), 0), [b"0 x"]), (lambda: planes(0, fp, ("glyphs",), sw, 5), [b"5 bytes per pixel"]),
                            (lambda: full(0, cap - 1), [b"capacity %d" % (cap - 1)]), (lambda: delta(0, cap - 1), [b"capacity %d" % (cap - 1)]),
                            (lambda: full(0, cap, fp, 16), [b"16"]), (lambda: full(0, cap, fp, 3, None), [b"NULL"]), (lambda: full(0, cap, fp, 3, p, None), [b"NULL"]),
                            (lambda: delta(0, cap, fp, 9), [b"merge_gap 9"]), (lambda: delta(0, cap, fp, 2, 256), [b"tolerance 256"])]:
            rc = call()
            msg = L.ycge_last_error(v.ctx)
            assert rc == abi.YCGE_ERR_INVALID_ARG and all(w_ in msg for w_ in words), msg
        assert L.ycge_video_blit_quadrants(None, fp, sw, sh, bpp, *ptrs(), 0) == abi.YCGE_ERR_INVALID_ARG
        assert (out == CANARY).all() and n.value == 12345 and list(info) == [9, 9, 9, 9]
        assert all((a == (CANARY if a.dtype != np.float32 else 7.0)).all() for a in arrs.values())
        # the next valid calls succeed, and the refusals forced no keyframe
        s = video_step(v, w1, s, False, "a refused call forces no keyframe")
        assert_planes(v.TryFlipAndBlitQuadrants(w1["frame"], quad_sdr=True, sdr=True, min_contrast=8), w1, 8, "after the refusals")


@pytest.mark.parametrize("ss", [1, 3])
def test_an_odd_super_sample_is_refused(lib, ss):
    fw, fh = 16, 8
    with VideoRenderer(fw, fh, ss, lib=lib) as v:
        f = I.noise(12, 10, 3)
        _, info = v.TryFlipAndBlitAnsiRgbDelta(f, fw, fh)
        assert info["keyframe"] == 1
        for call in (lambda: v.TryFlipAndBlitQuadrants(f), lambda: v.TryFlipAndBlitAnsiQuad(f, fw, fh), lambda: v.TryFlipAndBlitAnsiQuadDelta(f, fw, fh)):
            with pytest.raises(abi.YcgeError) as e:
                call()
            assert e.value.status == abi.YCGE_ERR_INVALID_ARG and f"super_sample {ss}" in str(e.value), str(e.value)
        _, info = v.TryFlipAndBlitAnsiRgbDelta(f, fw, fh)
        assert info["keyframe"] == 0, "the refusals left the context and its delta state alone"
        v.Resize(fw, fh, 2)
        got = v.TryFlipAndBlitQuadrants(f, quad_sdr=True, sdr=True)
        w_sdr, w_quad = VQ.blit_quadrants(f, 12, 10, 3, fw, fh, 2)
        assert_bits(got["sdr"], w_sdr, "after ycge_resize"); assert_bits(got["quad_sdr"], w_quad, "after ycge_resize")
        assert np.array_equal(got["glyphs"], Q.planes(w_quad, fw, fh)[0])
