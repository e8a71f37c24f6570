"""The delta sixel streams and Video mode's pixel plane without a GPU: the contract's known answers through ycge_sixel_encode_delta_host, the
restatement (tests/sixel_delta_restatement.py) against its interpreter and the host encoder against the restatement on the planes of
tests/sixel_delta_planes.py, the bound, the full-body identity, the super_sample 1 identity between the two restatements, the refusals -
and the plain C++ encoders once more as a stand-alone program under the host sanitizers (tests/sixel_host_main.cpp)."""
import ctypes as C
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import chexel_restatement as CR
import sixel_delta_planes as DP
import sixel_delta_restatement as D
import sixel_planes as P
import sixel_restatement as X
import video_quadrant_inputs as I
import video_restatement as VR

ROOT = Path(__file__).resolve().parents[1]
U8P, U32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
EXPORTS = ("ycge_video_blit_pixels", "ycge_video_blit_sixel", "ycge_render_frame_sixel_delta", "ycge_video_blit_sixel_delta", "ycge_sixel_encode_delta_host")
HOOKS = ("ycge_test_video_pixels", "ycge_test_sixel_delta_stream")
KNOWN = DP.KNOWN
# (edits to the known picture, the body, the stream's bytes, out_info)
KNOWN_ANSWERS = [
    ([((6, 2), 0), ((6, 3), 7)], b"-#0??@$#7???@", 3165, (0, 1, 2, 2)),
    ([((1, 1), 0), ((2, 3), 215)], b"#0?zxx$#7?CEA$#215???C", 3174, (0, 1, 18, 3)),
    ([], b"", 3152, (0, 0, 0, 0)),
]


@pytest.fixture(scope="module")
def lib(product_lib):
    """the exports, looked up first: a library without them fails here, it does not skip"""
    for n in EXPORTS + HOOKS:
        assert getattr(product_lib, n) is not None
    return product_lib


def host_delta(L, prev, cur, viewport=(0, 0)):
    """ycge_sixel_encode_delta_host into a buffer of the bound's size with a canary behind it: (the stream's bytes, info)"""
    prev, cur = np.ascontiguousarray(prev, np.uint8), np.ascontiguousarray(cur, np.uint8)
    H, W = cur.shape
    cap = X.bound(W, H)
    out, n, info = np.full(cap + 64, P.CANARY, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)(9, 9, 9, 9)
    rc = L.ycge_sixel_encode_delta_host(prev.ctypes.data_as(U8P), cur.ctypes.data_as(U8P), W, H, viewport[0], viewport[1], out.ctypes.data_as(U8P), cap, C.byref(n), info)
    assert rc == 0, rc
    assert n.value <= cap and (out[n.value:] == P.CANARY).all(), "bytes past the stream's length were written"
    return out[:n.value].tobytes(), tuple(info)


def edited(edits):
    cur = KNOWN.copy()
    for (y, x), v in edits:
        cur[y, x] = v
    return cur


@pytest.mark.parametrize("k", range(len(KNOWN_ANSWERS)))
def test_known_answers(lib, k):
    edits, body, size, info = KNOWN_ANSWERS[k]
    cur = edited(edits)
    head = b"\x1b[2;3H\x1bP0;1q\"1;1;5;7" + X.register_definitions()
    want = head + body + b"\x1b\\"
    assert len(want) == size
    assert D.encode_delta(KNOWN, cur, (2, 1)) == (want, info)
    assert host_delta(lib, KNOWN, cur, (2, 1)) == (want, info)
    plane, painted = D.apply(want, KNOWN, cur)
    assert np.array_equal(plane, cur) and int(painted.sum()) <= info[2]


def test_apply_refuses_what_a_delta_must_not_do():
    cur = edited(KNOWN_ANSWERS[0][0])
    s, _ = D.encode_delta(KNOWN, cur, (2, 1))
    assert np.array_equal(D.apply(s, KNOWN, cur)[0], cur)
    with pytest.raises(AssertionError, match="twice"):
        D.apply(s.replace(b"#7???@", b"#7??@@"), KNOWN, cur)
    with pytest.raises(AssertionError, match="outside"):
        D.apply(s.replace(b"-#0??@", b"-#0@?@"), KNOWN, cur)
    with pytest.raises(AssertionError, match="unpainted"):
        D.apply(s.replace(b"$#7???@", b""), KNOWN, cur)
    # P2 = 1: a zero bit leaves the pixel - the interpreter starts from the screen, not from an empty plane
    assert np.array_equal(D.apply(D.encode_delta(KNOWN, KNOWN)[0], KNOWN, KNOWN)[0], KNOWN)


@pytest.mark.parametrize("w", DP.WIDTHS)
def test_pairs_restatement_interpreter_and_host_encoder(lib, w):
    for h in DP.HEIGHTS:
        for k, (name, prev, cur) in enumerate(DP.pairs(w, h)):
            vp = P.VIEWPORTS[k % len(P.VIEWPORTS)]
            want, info = D.encode_delta(prev, cur, vp)
            plane, painted = D.apply(want, prev, cur)
            assert np.array_equal(plane, cur), (w, h, name)
            assert int(painted.sum()) <= info[2] <= w * h and len(want) <= X.bound(w, h), (w, h, name)
            assert host_delta(lib, prev, cur, vp) == (want, info), (w, h, name)


def test_300_bands(lib):
    for name, prev, cur in DP.bands_300():
        want, info = D.encode_delta(prev, cur, (9, 99))
        assert np.array_equal(D.apply(want, prev, cur)[0], cur), name
        assert host_delta(lib, prev, cur, (9, 99)) == (want, info), name
    assert D.encode_delta(*DP.bands_300()[0][1:])[1][1] == 3


def test_bound_holds_for_adversarial_planes_up_to_9_by_13(lib):
    """the delta's bound (csrc/ycge_sixel_host.cpp): the header 3 bytes longer, an empty band one byte out of a budget of at least 36"""
    for w in range(1, 10):
        for h in range(1, 14):
            assert X.bound(w, h) - 3200 >= 36 * -(-h // 6)
            for prev, cur in DP.adversarial(w, h):
                s, info = host_delta(lib, prev, cur, (999999, 999999))
                assert len(s) <= X.bound(w, h), (w, h, len(s))
                assert (s, info) == D.encode_delta(prev, cur, (999999, 999999)), (w, h)
    assert len(D.delta_header(5, 7, (2, 1))) == len(X.encode(KNOWN, (2, 1)).split(b"#0~")[0]) + 3


@pytest.mark.parametrize("w,h", [(1, 1), (5, 7), (64, 6), (65, 13), (129, 13)])
def test_everything_changed_is_the_full_body(lib, w, h):
    name, prev, cur = DP.pairs(w, h)[-1]
    assert name == "everything_changed" and (prev != cur).all()
    s, info = host_delta(lib, prev, cur, (3, 4))
    full = X.encode(cur, (3, 4))
    head = len(D.delta_header(w, h, (3, 4)))
    assert s[head:] == full[head - 3:] and info[:3] == (0, -(-h // 6), w * h)


@pytest.mark.parametrize("case", [(200, 40, 3, 7, 5), (7, 5, 4, 65, 3), (1, 1, 3, 1, 1), (40, 30, 4, 20, 5)])
def test_super_sample_1_rgba_is_the_blit_s_rgba(case):
    """between the two restatements: at super_sample 1 a half-cell is one sample, so Video mode's pixel plane is ycge_video_blit's out_rgba"""
    sw, sh, bpp, fw, fh = case
    for f in (I.noise(sw, sh, bpp), I.drawn(sw, sh, bpp) if sw > 4 else I.constant(sw, sh, bpp, 255)):
        rgba, index = D.video_pixels(f, sw, sh, bpp, fw, fh, 1)
        assert np.array_equal(rgba, CR.encode(VR.blit(f, sw, sh, bpp, fw, fh, 1))[2]), case
        assert np.array_equal(index, X.quantise(rgba[..., :3]))
        assert rgba.shape == (2 * fh, fw, 4) and (rgba[..., 3] == 255).all()


def test_refusals_of_the_host_encoder(lib):
    L = lib
    prev, cur = np.ascontiguousarray(KNOWN), np.ascontiguousarray(edited(KNOWN_ANSWERS[0][0]))
    cap = X.bound(5, 7)
    out, n = np.zeros(cap, np.uint8), C.c_size_t(0)
    a, b, o = prev.ctypes.data_as(U8P), cur.ctypes.data_as(U8P), out.ctypes.data_as(U8P)
    call = lambda p=a, q=b, w=5, h=7, vx=0, vy=0, dst=o, c=cap, ln=C.byref(n): L.ycge_sixel_encode_delta_host(p, q, w, h, vx, vy, dst, c, ln, None)
    bad = cur.copy(); bad[6, 4] = 216
    for rc in (call(p=None), call(q=None), call(dst=None), call(ln=None), call(w=0), call(h=0), call(w=-5), call(vx=-1), call(vy=-1), call(c=cap - 1),
               call(q=bad.ctypes.data_as(U8P)), call(p=bad.ctypes.data_as(U8P)), call(w=2 ** 20, h=2 ** 20)):
        assert rc != 0
    assert not out.any() and n.value == 0
    assert call() == 0 and n.value == 3165          # (out_info may be NULL)


def test_exports_and_hooks_resolve(lib):
    from yetanotherconsolegameengine_amd import abi, build
    header = (ROOT / "include" / "ycge.h").read_text(encoding="utf-8")
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert n in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", header), n
    assert tuple(abi.SIXEL_DELTA_HOOK_PROTOTYPES) == HOOKS
    for n in HOOKS:
        assert n not in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", hooks) and ("int " + n + "(") not in header, n
    assert "#define YCGE_ABI_VERSION 10" in header
    assert "k_video_blit keeps no per-sample plane" not in header and "partial or delta images" not in header
    assert "ycge_sixel_host.cpp" in build.SOURCES
    # refusals that need no device: a NULL context
    assert lib.ycge_render_frame_sixel_delta(None, 0, 0, 0, 0, 0, None, 0, None, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    assert lib.ycge_video_blit_pixels(None, None, 1, 1, 3, None, None, None, 0) == abi.YCGE_ERR_INVALID_ARG
    assert lib.ycge_video_blit_sixel(None, None, 1, 1, 3, 0, 0, 0, 0, None, 0, None, None) == abi.YCGE_ERR_INVALID_ARG
    assert lib.ycge_video_blit_sixel_delta(None, None, 1, 1, 3, 0, 0, 0, 0, 0, None, 0, None, None, None) == abi.YCGE_ERR_INVALID_ARG
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert n + "(" in cs, n


def test_host_encoders_under_the_sanitizers(tmp_path):
    """csrc/ycge_sixel_host.cpp is free of HIP and of the context: a stand-alone program over it, built with -fsanitize=address,undefined, runs
    the known answers, the seam planes and the delta pairs; its streams are the restatement's and the sanitizers report nothing"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "sixel_host_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "sixel_host_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    jobs = []          # (cur, prev or None, viewport, clear)
    for edits, *_ in KNOWN_ANSWERS:
        jobs.append((edited(edits), KNOWN, (2, 1), False))
    jobs.append((KNOWN, None, (2, 1), True))
    for name in sorted(P.SEAMS):
        plane = P.SEAMS[name]()
        jobs.append((plane, None, (9, 99), True))
        jobs.append((plane, np.roll(plane, 1, axis=1), (9, 99), False))
    for w, h in ((1, 1), (5, 7), (65, 13), (1025, 7)):
        jobs += [(cur, prev, (0, 0), False) for _, prev, cur in DP.pairs(w, h)]
    jobs += [(cur, prev, (0, 0), False) for _, prev, cur in DP.bands_300()]
    with open(tmp_path / "jobs", "wb") as f:
        for cur, prev, vp, clear in jobs:
            f.write(struct.pack("<6i", cur.shape[1], cur.shape[0], vp[0], vp[1], int(clear), int(prev is not None)))
            f.write(np.ascontiguousarray(cur, np.uint8).tobytes())
            if prev is not None:
                f.write(np.ascontiguousarray(prev, np.uint8).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "jobs"), str(tmp_path / "streams")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "%d jobs" % len(jobs)
    data, at = (tmp_path / "streams").read_bytes(), 0
    for k, (cur, prev, vp, clear) in enumerate(jobs):
        rc, n, *info = struct.unpack_from("<iQ4I", data, at)
        at += 28
        got = data[at:at + n]
        at += n
        assert rc == 0, k
        if prev is None:
            assert got == X.encode(cur, vp, clear), k
        else:
            assert (got, tuple(info)) == D.encode_delta(prev, cur, vp), k
    assert at == len(data)
