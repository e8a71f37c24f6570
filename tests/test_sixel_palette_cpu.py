"""The adaptive sixel palette without a GPU: the restatement (tests/sixel_palette_restatement.py) on the contract's known answer and through
the independent sixel interpreter, the library's plain C++ (ycge_sixel_palette_host, ycge_sixel_encode_palette_host, the bound) held to it on
the planes of tests/sixel_palette_planes.py, the refusals - and the plain C++ once more as a stand-alone program under the host sanitizers
(tests/sixel_palette_host_main.cpp).  Every comparison is exact."""
import ctypes as C
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sixel_palette_planes as PP
import sixel_palette_restatement as R

ROOT = Path(__file__).resolve().parents[1]
U8P, I32P = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
EXPORTS = ("ycge_sixel_palette_stream_bound", "ycge_render_frame_sixel_palette", "ycge_video_blit_sixel_palette", "ycge_render_frame_pixels_palette",
           "ycge_video_blit_pixels_palette", "ycge_sixel_palette_host", "ycge_sixel_encode_palette_host")
HOOKS = ("ycge_test_sixel_palette", "ycge_test_sixel_palette_stream")
KNOWN = b"\x1b[1;1H\x1bPq\"1;1;6;12#0;2;0;0;0#1;2;100;100;100#0!6~-#1!6~\x1b\\"


@pytest.fixture(scope="module")
def lib(product_lib):
    """the exports, looked up first: a library without them fails here, it does not skip"""
    for n in EXPORTS + HOOKS:
        assert getattr(product_lib, n) is not None
    return product_lib


def host_palette(L, rgba):
    """ycge_sixel_palette_host with a canary behind every output: (index, palette, pct, n)"""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    H, W = rgba.shape[:2]
    index, palette, pct, n = np.full(W * H + 16, PP.CANARY, np.uint8), np.full(1024 + 16, PP.CANARY, np.uint8), np.full(768 + 16, PP.CANARY, np.uint8), C.c_int32(-1)
    rc = L.ycge_sixel_palette_host(rgba.ctypes.data_as(U8P), W, H, index.ctypes.data_as(U8P), palette.ctypes.data_as(U8P), pct.ctypes.data_as(U8P), C.byref(n))
    assert rc == 0, rc
    for a, size in ((index, W * H), (palette, 1024), (pct, 768)):
        assert (a[size:] == PP.CANARY).all(), "bytes past an output were written"
    return index[:W * H].reshape(H, W), palette[:1024].reshape(256, 4), pct[:768].reshape(256, 3), n.value


def host_encode(L, index, pct, n, viewport=(0, 0), clear=False):
    """ycge_sixel_encode_palette_host into a buffer of the bound's size with a canary behind it: the stream's bytes"""
    index, pct = np.ascontiguousarray(index, np.uint8), np.ascontiguousarray(pct, np.uint8)
    H, W = index.shape
    cap = R.bound(W, H)
    out, ln = np.full(cap + 64, PP.CANARY, np.uint8), C.c_size_t(0)
    rc = L.ycge_sixel_encode_palette_host(index.ctypes.data_as(U8P), pct.ctypes.data_as(U8P), n, W, H, viewport[0], viewport[1], int(clear), out.ctypes.data_as(U8P), cap,
                                          C.byref(ln))
    assert rc == 0, rc
    assert ln.value <= cap and (out[ln.value:] == PP.CANARY).all(), "bytes past the stream's length were written"
    return out[:ln.value].tobytes()


def test_known_answer():
    s, index, palette, pct, n, _ = R.stream(PP.plane("6x12_two"))
    assert s == KNOWN and n == 2
    assert palette[:2].tolist() == [[0, 0, 0, 255], [255, 255, 255, 255]] and not palette[2:].any() and not pct[2:].any()
    shown, vp, clear, defined = R.shown(s)
    assert vp == (0, 0) and not clear and defined == 2 and np.array_equal(shown, pct.astype(np.int64)[index])


def test_known_answer_of_the_host_functions(lib):
    index, palette, pct, n = host_palette(lib, PP.plane("6x12_two"))
    assert n == 2 and host_encode(lib, index, pct, n) == KNOWN


@pytest.mark.parametrize("name", sorted(PP.PLANES))
def test_restatement_on_the_planes(name):
    """what the rule promises of every plane: the counts checked by hand, a total table, registers that hold pixels, a stream the
    interpreter paints exactly once a pixel with pct[index], under the bound"""
    s, index, palette, pct, n, table = PP.expected(name)
    rgba = PP.plane(name)
    if name in PP.COUNTS:
        assert n == PP.COUNTS[name]
    assert 1 <= n <= 256 and table.max() == n - 1 and sorted(np.unique(index).tolist()) == list(range(n)), "every register holds pixels"
    assert (palette[:n, 3] == 255).all() and not palette[n:].any() and not pct[n:].any() and pct.max() <= 100
    shown, vp, clear, defined = R.shown(s)
    assert defined == n and np.array_equal(shown, pct.astype(np.int64)[index])
    assert len(s) <= R.bound(rgba.shape[1], rgba.shape[0])
    # a register's bytes lie within its pixels' range: a mean
    for i in range(n):
        px = rgba[index == i][:, :3]
        assert (palette[i, :3] >= px.min(axis=0)).all() and (palette[i, :3] <= px.max(axis=0)).all(), i


def test_the_rule_where_it_decides():
    # the clamp: the lone pixel is cut from the hundred, c = omax - 1
    _, index, palette, _, n, table = PP.expected("clamp")
    assert n == 2 and index[0, 0] == 0 and (index[0, 1:] == 1).all() and table[1 << 10 | 5 << 5 | 5] == 0 and table[24 << 10] == 0 and table[25 << 10] == 1
    # ties: g before b with r flat; r first with all three equal - the second register is the first cut's upper half
    _, index, *_ = PP.expected("ties_two")
    assert index.tolist() == [[0, 2], [1, 3]]
    _, index, palette, *_ = PP.expected("ties_three")
    assert palette[1, 0] == 104 and palette[0, 0] == 8 and index[1, 0] == 1 and index[0, 0] == 0


@pytest.mark.parametrize("name", sorted(PP.PLANES))
def test_host_functions_against_the_restatement(lib, name):
    for k in range(2):
        s, index, palette, pct, n, _ = PP.expected(name, k)
        got = host_palette(lib, PP.plane(name))
        assert got[3] == n and np.array_equal(got[0], index) and np.array_equal(got[1], palette) and np.array_equal(got[2], pct), name
        assert host_encode(lib, got[0], got[2], got[3], PP.VIEWPORTS[k % 3], bool(k & 1)) == s, (name, k)


def test_hold_in_the_restatement():
    first, second = PP.hold_pair()
    _, _, palette, pct, n, table = R.stream(first)
    held = (table, palette, pct, n)
    s, index, *_ = R.stream(second, (2, 1), True, held)
    own = R.stream(second, (2, 1), True)
    assert (R.build(first)[0] != own[5]).any(), "the second picture's own palette differs"
    empty = np.bincount(R.bins_of(first), minlength=R.BINS) == 0
    assert empty[R.bins_of(second)].any(), "pixels in bins the first left empty"
    shown, *_ = R.shown(s)
    assert np.array_equal(shown, pct.astype(np.int64)[index]) and index.max() < n


def test_bound(lib):
    n = C.c_size_t(0)
    for w, h in [(1, 1), (5, 7), (42, 6), (43, 6), (44, 7), (1920, 1072), (4097, 7), (8, 1800), (100000, 1), (1, 100000)]:
        assert lib.ycge_sixel_palette_stream_bound(w, h, C.byref(n)) == 0 and n.value == R.bound(w, h), (w, h)
    assert R.bound(1920, 1072) == 4700 + 179 * 256 * 1925
    w = next(w for w in range(1, 10 ** 6) if R.bound(w, 1072) >= 2 ** 32)
    for (gw, gh), ok in [((w - 1, 1072), True), ((w, 1072), False)]:
        assert R.fits(gw, gh) == ok and (lib.ycge_sixel_palette_stream_bound(gw, gh, C.byref(n)) == 0) == ok
    for gw, gh in [(0, 5), (5, 0), (-1, 5), (5, -6), (2 ** 31 - 1, 2 ** 31 - 1)]:
        assert lib.ycge_sixel_palette_stream_bound(gw, gh, C.byref(n)) != 0
    assert lib.ycge_sixel_palette_stream_bound(5, 7, None) != 0


def test_the_longest_streams_stay_under_the_bound():
    """the bound's reasoning: 256 definitions of 18 bytes, and lines of #ddd, W characters and a separator - every register in every band,
    sixels that defeat every run.  The longest stream the rule can make of a small W x H: min(W H, 256) registers, all three-digit"""
    for w, h in ((43, 6), (44, 12), (64, 7), (3, 2), (1, 1)):
        n = min(256, w * h)
        index = (np.arange(w * h).reshape(h, w) * 7 % n).astype(np.uint8)
        pct = np.full((256, 3), 100, np.uint8)
        s = R.encode(index, pct, n, (99999, 99999), True)
        assert len(s) <= R.bound(w, h), (w, h, len(s))
    assert len(R.definitions(np.full((256, 3), 100, np.uint8), 256)) == 10 * 16 + 90 * 17 + 156 * 18 <= 4608


def test_refusals_of_the_host_functions(lib):
    L = lib
    rgba = np.ascontiguousarray(PP.plane("6x12_two"))
    index, palette, pct, n = host_palette(L, rgba)
    idx, pc = np.ascontiguousarray(index), np.ascontiguousarray(pct)
    cap = R.bound(6, 12)
    out, ln = np.zeros(cap, np.uint8), C.c_size_t(0)
    p, q, o = idx.ctypes.data_as(U8P), pc.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
    call = lambda index=p, pct=q, count=2, w=6, h=12, vx=0, vy=0, dst=o, c=cap, l=C.byref(ln): L.ycge_sixel_encode_palette_host(index, pct, count, w, h, vx, vy, 0, dst, c, l)
    bad = idx.copy(); bad[11, 5] = 2
    worse = pc.copy(); worse[1, 2] = 101
    for rc in (call(index=None), call(pct=None), call(dst=None), call(l=None), call(count=0), call(count=257), call(count=1), call(w=0), call(h=0), call(vx=-1),
               call(vy=-1), call(c=cap - 1), call(index=bad.ctypes.data_as(U8P)), call(pct=worse.ctypes.data_as(U8P)), call(w=2 ** 20, h=2 ** 20)):
        assert rc != 0
    assert not out.any() and ln.value == 0
    assert call() == 0 and out[:ln.value].tobytes() == KNOWN
    r = rgba.ctypes.data_as(U8P)
    cnt = C.c_int32(-7)
    for rc in (L.ycge_sixel_palette_host(None, 6, 12, None, None, None, C.byref(cnt)), L.ycge_sixel_palette_host(r, 0, 12, None, None, None, C.byref(cnt)),
               L.ycge_sixel_palette_host(r, 6, -1, None, None, None, C.byref(cnt)), L.ycge_sixel_palette_host(r, 6, 12, None, None, None, None),
               L.ycge_sixel_palette_host(r, 4097, 4096, None, None, None, C.byref(cnt))):
        assert rc != 0 and cnt.value == -7
    assert L.ycge_sixel_palette_host(r, 6, 12, None, None, None, C.byref(cnt)) == 0 and cnt.value == 2


def test_exports_and_hooks_resolve(lib):
    from yetanotherconsolegameengine_amd import abi, build
    header = (ROOT / "include" / "ycge.h").read_text(encoding="utf-8")
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert n in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", header), n
    assert tuple(abi.SIXEL_PALETTE_HOOK_PROTOTYPES) == HOOKS
    for n in HOOKS:
        assert n not in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", hooks) and ("int " + n + "(") not in header, n
    assert "#define YCGE_ABI_VERSION 10" in header
    assert "or an adaptive palette" not in header and "a grey ramp" in header
    assert "ycge_sixel_palette.hip" in build.SOURCES
    # refusals that need no device: a NULL context
    assert lib.ycge_render_frame_sixel_palette(None, 0, 0, 0, 0, None, 0, None, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    assert lib.ycge_render_frame_pixels_palette(None, None, None, None, 0, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    assert lib.ycge_video_blit_sixel_palette(None, None, 1, 1, 3, 0, 0, 0, 0, None, 0, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    assert lib.ycge_video_blit_pixels_palette(None, None, 1, 1, 3, None, None, None, 0, None, None) == abi.YCGE_ERR_INVALID_ARG
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert n + "(" in cs, n
    wrapper = (ROOT / "bindings" / "csharp" / "HipRaytraceWrapper.cs").read_text(encoding="utf-8")
    video = (ROOT / "bindings" / "csharp" / "HipVideoWrapper.cs").read_text(encoding="utf-8")
    for text, call in ((wrapper, "Ycge.ycge_render_frame_sixel_palette("), (video, "Ycge.ycge_video_blit_sixel_palette(")):
        assert "SixelAdaptivePalette" in text and "SixelHoldPalette" in text and call in text


def test_plain_cpp_under_the_sanitizers(tmp_path):
    """csrc/ycge_sixel_host.cpp is free of HIP and of the context: a stand-alone program over it, built with -fsanitize=address,undefined, runs
    the planes and the hold pair; its registers, palettes and streams are the restatement's and the sanitizers report nothing"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sixel_palette_host_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                        str(ROOT / "tests" / "sixel_palette_host_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    jobs = [(PP.plane(name), PP.VIEWPORTS[k % 3], bool(k & 1), False, PP.expected(name, k)) for k, name in enumerate(sorted(PP.PLANES))]
    first, second = PP.hold_pair()
    built = R.stream(first)
    jobs.append((first, (0, 0), False, False, built))
    jobs.append((second, (2, 1), True, True, R.stream(second, (2, 1), True, (built[5], built[2], built[3], built[4]))))
    with open(tmp_path / "jobs", "wb") as f:
        for rgba, vp, clear, hold, _ in jobs:
            f.write(struct.pack("<6i", rgba.shape[1], rgba.shape[0], vp[0], vp[1], int(clear), int(hold)))
            f.write(np.ascontiguousarray(rgba, np.uint8).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "jobs"), str(tmp_path / "results")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "%d jobs" % len(jobs)
    data, at = (tmp_path / "results").read_bytes(), 0
    for k, (rgba, vp, clear, hold, want) in enumerate(jobs):
        rc, n, length = struct.unpack_from("<iiQ", data, at)
        at += 16
        px = rgba.shape[0] * rgba.shape[1]
        palette, pct, index = data[at:at + 1024], data[at + 1024:at + 1792], data[at + 1792:at + 1792 + px]
        at += 1792 + px
        got = data[at:at + length]
        at += length
        s, w_index, w_palette, w_pct, w_n, _ = want
        assert rc == 0 and n == w_n, k
        assert palette == w_palette.tobytes() and pct == w_pct.tobytes() and index == w_index.tobytes() and got == s, k
    assert at == len(data)
