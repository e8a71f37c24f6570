"""The sixel frames without a GPU: the restatement (tests/sixel_restatement.py) on the contract's known answer, its interpreter against its
encoder, and the library's host encoder, bound and refusals held to it.  sixel_planes.py draws and builds the planes both test files use."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import sixel_planes as P
import sixel_restatement as X

ROOT = Path(__file__).resolve().parents[1]
U8P = C.POINTER(C.c_uint8)
EXPORTS = ("ycge_sixel_stream_bound", "ycge_render_frame_pixels", "ycge_render_frame_sixel", "ycge_sixel_encode_host")
HOOKS = ("ycge_test_pixels", "ycge_test_sixel_stream")
KNOWN = np.array([[0, 0, 0, 0, 215], [0, 7, 7, 7, 7], [0, 7, 7, 7, 7], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [43, 43, 43, 43, 0]], np.uint8)
KNOWN_BODY = b"#0~xxxw$#7?!4E$#215!4?@-#0!4?@$#43!4@\x1b\\"


def host_encode(L, plane, viewport=(0, 0), clear=False):
    """ycge_sixel_encode_host into a buffer of the bound's size with a canary behind it: the stream's bytes"""
    plane = np.ascontiguousarray(plane, np.uint8)
    H, W = plane.shape
    cap = X.bound(W, H)
    out, n = np.full(cap + 64, P.CANARY, np.uint8), C.c_size_t(0)
    rc = L.ycge_sixel_encode_host(plane.ctypes.data_as(U8P), W, H, viewport[0], viewport[1], int(clear), out.ctypes.data_as(U8P), cap, C.byref(n))
    assert rc == 0, rc
    assert n.value <= cap and (out[n.value:] == P.CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes()


def test_known_answer_of_the_restatement():
    s = X.encode(KNOWN, (2, 1), True)
    head = b"\x1b[2J\x1b[2;3H\x1bPq\"1;1;5;7"
    assert s.startswith(head + b"#0;2;0;0;0#1;2;0;0;20#2;2;0;0;40") and s.endswith(b"#215;2;100;100;100" + KNOWN_BODY)
    assert len(X.register_definitions()) == 3130 and len(s) == 3190
    plane, vp, clear, palette = X.decode(s)
    assert np.array_equal(plane, KNOWN) and vp == (2, 1) and clear
    assert len(palette) == 216 and palette[43] == (20, 20, 20) and palette[7] == (0, 20, 20) and palette[215] == (100, 100, 100)


def test_known_answer_of_the_host_encoder(product_lib):
    assert host_encode(product_lib, KNOWN, (2, 1), True) == X.encode(KNOWN, (2, 1), True)
    assert host_encode(product_lib, KNOWN, (2, 1), True).endswith(KNOWN_BODY)


def test_decode_refuses_a_pixel_painted_twice_or_never():
    s = X.encode(KNOWN)
    with pytest.raises(AssertionError, match="twice"):
        X.decode(s.replace(b"#7?!4E", b"#7~!4E"))
    with pytest.raises(AssertionError, match="unpainted"):
        X.decode(s.replace(b"#7?!4E", b"#7?!3E"))


@pytest.mark.parametrize("w,h", [(w, h) for w in (1, 3, 4, 5, 9, 10, 11, 63, 64, 65) for h in P.HEIGHTS] + [(w, h) for w in (99, 100, 101, 127, 128, 129, 255, 256, 257) for h in (6, 7)])
def test_drawn_planes_round_trip_and_the_host_encoder_agrees(product_lib, w, h):
    for k, plane in enumerate(P.drawn(w, h)):
        vp, clear = P.VIEWPORTS[k % len(P.VIEWPORTS)], bool(k & 1)
        want = X.encode(plane, vp, clear)
        got_plane, got_vp, got_clear, _ = X.decode(want)
        assert np.array_equal(got_plane, plane) and got_vp == vp and got_clear == clear, (w, h, k)
        assert len(want) <= X.bound(w, h)
        assert host_encode(product_lib, plane, vp, clear) == want, (w, h, k)


@pytest.mark.parametrize("name", sorted(P.SEAMS))
def test_seam_planes_round_trip_and_the_host_encoder_agrees(product_lib, name):
    plane = P.SEAMS[name]()
    want = X.encode(plane, (9, 99), True)
    assert np.array_equal(X.decode(want)[0], plane), name
    assert len(want) <= X.bound(plane.shape[1], plane.shape[0])
    assert host_encode(product_lib, plane, (9, 99), True) == want, name


def test_the_longest_lines_stay_under_the_bound():
    """the bound's reasoning: a line is at most #ddd, W characters and a separator - alternating sixels defeat every run"""
    for w, h in ((36, 6), (37, 12), (200, 6)):
        plane = (np.arange(w * h).reshape(h, w) * 7 % 216).astype(np.uint8)
        assert len(X.encode(plane, (999, 999), True)) <= X.bound(w, h)


def test_bound_against_the_restatement(product_lib):
    n = C.c_size_t(0)
    for w, h in [(1, 1), (5, 7), (35, 6), (36, 6), (37, 7), (1920, 1072), (4097, 7), (8, 1800), (100000, 1), (1, 100000)]:
        assert product_lib.ycge_sixel_stream_bound(w, h, C.byref(n)) == 0 and n.value == X.bound(w, h), (w, h)
    assert X.bound(1920, 1072) == 3200 + 179 * 216 * 1925
    # the first geometry whose bound passes 2^32, by width at 1072 rows and by height at 1920 columns
    w = next(w for w in range(1, 10 ** 6) if X.bound(w, 1072) >= 2 ** 32)
    h = next(h for h in range(1, 10 ** 7, 6) if X.bound(1920, h) >= 2 ** 32)
    for (gw, gh), ok in [((w - 1, 1072), True), ((w, 1072), False), ((1920, h - 1), True), ((1920, h), False)]:
        assert X.fits(gw, gh) == ok
        rc = product_lib.ycge_sixel_stream_bound(gw, gh, C.byref(n))
        assert (rc == 0) == ok and (not ok or n.value == X.bound(gw, gh)), (gw, gh)
    for gw, gh in [(0, 5), (5, 0), (-1, 5), (5, -6), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert product_lib.ycge_sixel_stream_bound(gw, gh, C.byref(n)) != 0
    assert product_lib.ycge_sixel_stream_bound(5, 7, None) != 0


def test_quantiser_range_and_nearest_level():
    v = np.arange(256)
    plain = (v + 25) // 51
    assert plain.min() == 0 and plain.max() == 5
    assert (np.abs(plain * 51 - v) == np.abs(np.arange(6)[:, None] * 51 - v).min(axis=0)).all(), "dither 0 picks the nearest cube level"
    for d in range(16):
        level = (32 * v + 102 * d + 51) // 1632
        assert level.min() == 0 and level.max() == 5 and (np.diff(level) >= 0).all(), d
    grey = np.stack([v, v, v], axis=-1).reshape(16, 16, 3)
    assert (X.quantise(grey, 0) % 43 == 0).all() and (X.quantise(grey, 1) % 43 == 0).all()
    assert X.quantise(np.array([[[255, 0, 128]]]), 0)[0, 0] == 36 * 5 + 0 + 3
    assert sorted(X.BAYER.ravel().tolist()) == list(range(16))
    # the matrix is indexed by the hi-res pixel, rows by y: byte 26 rounds up only under the larger entries
    y, x = np.mgrid[0:4, 0:4]
    assert np.array_equal(X.quantise(np.full((4, 4, 3), 26), 1) // 43, (32 * 26 + 102 * X.BAYER[y, x] + 51) // 1632)


def test_host_encoder_refusals(product_lib):
    L = product_lib
    plane = np.ascontiguousarray(KNOWN)
    cap = X.bound(5, 7)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    p, o = plane.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
    call = lambda index=p, w=5, h=7, vx=0, vy=0, dst=o, c=cap, ln=C.byref(n): L.ycge_sixel_encode_host(index, w, h, vx, vy, 0, dst, c, ln)
    bad = plane.copy(); bad[6, 4] = 216
    for rc in (call(index=None), call(dst=None), call(ln=None), call(w=0), call(h=0), call(w=-5), call(vx=-1), call(vy=-1), call(c=cap - 1),
               call(index=bad.ctypes.data_as(U8P)), call(w=2 ** 20, h=2 ** 20)):
        assert rc != 0
    assert not out.any() and n.value == 0
    assert call() == 0 and n.value == len(X.encode(KNOWN))


def test_exports_and_hooks_resolve(product_lib):
    from yetanotherconsolegameengine_amd import abi, build
    header = (ROOT / "include" / "ycge.h").read_text(encoding="utf-8")
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert hasattr(product_lib, n) and n in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", header), n
    assert tuple(abi.SIXEL_HOOK_PROTOTYPES) == HOOKS
    for n in HOOKS:
        assert hasattr(product_lib, n) and n not in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", hooks) and ("int " + n + "(") not in header, n
    assert "#define YCGE_ABI_VERSION 10" in header
    assert {"ycge_sixel.cpp", "ycge_sixel.hip"} <= set(build.SOURCES)
    # refusals that need no device: a NULL context
    assert product_lib.ycge_render_frame_pixels(None, None, None, None, 0, None) == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_render_frame_sixel(None, 0, 0, 0, 0, None, 0, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    cs = (ROOT / "bindings" / "csharp" / "HipRaytraceWrapper.cs").read_text(encoding="utf-8")
    assert "SixelGraphics" in cs and "SixelDither" in cs and "Ycge.ycge_render_frame_sixel(" in cs
