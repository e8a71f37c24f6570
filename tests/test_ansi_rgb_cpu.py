"""The 24-bit colour ANSI streams without a GPU: known answers of their restatement (tests/ansi_rgb_restatement.py), the terminal
equivalence that ties a delta to the full stream - exactly with tolerance 0, within the tolerance otherwise, and never accumulating - the
length bound, the library's ycge_ansi_rgb_stream_bound, and the surface of the new exports."""
import ctypes as C
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import ansi_rgb_restatement as R
from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
UH = R.UPPER_HALF.encode("utf-8")
END = b"\x1b[0m"
EXPORTS = ("ycge_ansi_rgb_stream_bound", "ycge_render_frame_ansi_rgb", "ycge_render_frame_ansi_rgb_delta", "ycge_video_blit_ansi_rgb",
           "ycge_video_blit_ansi_rgb_delta")


def plane(cells):
    """rows of (fg triple, bg triple) chexels -> the RGBA plane (2 fbH, fbW, 4), the fourth byte 255"""
    h, w = len(cells), len(cells[0])
    p = np.full((2 * h, w, 4), 255, np.uint8)
    for y, row in enumerate(cells):
        for x, (fg, bg) in enumerate(row):
            p[2 * y, x, :3], p[2 * y + 1, x, :3] = fg, bg
    return p


def both(fg, bg):
    return b"\x1b[38;2;%d;%d;%d;48;2;%d;%d;%dm" % (tuple(fg) + tuple(bg))


def fg_only(c):
    return b"\x1b[38;2;%d;%d;%dm" % tuple(c)


def bg_only(c):
    return b"\x1b[48;2;%d;%d;%dm" % tuple(c)


A1, B1, A2, B2 = (1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12)
FAR = ((200, 200, 200), (201, 201, 201))


# ------------------------------------------------------------------------------------------------------------- known answers
def test_the_default_colours_are_the_encoder_on_the_palette():
    pal = R.palette_rgb()
    assert pal[0] == (0, 0, 0) and pal[15] == (255, 255, 255) and pal[7] == (225, 225, 225) and pal[8] == (188, 188, 188) and pal[4] == (188, 0, 0)


def test_one_by_one_console():
    cur = plane([[(A1, B1)]])
    want = b"\x1b[1;1H" + both(A1, B1) + UH + END
    got, info, shown = R.delta(cur, cur, 1, 1)
    assert (got, info) == (want, dict(keyframe=0, changed=0, emitted=1, runs=1)) and (shown == cur).all()          # the last cell, always
    got, info, shown = R.delta(plane([[FAR]]), cur, 1, 1)
    assert (got, info) == (want, dict(keyframe=0, changed=1, emitted=1, runs=1)) and (shown == cur).all()
    got, info, shown = R.delta(None, cur, 1, 1)
    assert got == R.stream(cur, 1, 1) == want and info == dict(keyframe=1, changed=0, emitted=0, runs=0) and (shown == cur).all()
    assert R.stream(cur, 1, 1, clear=True) == b"\x1b[2J\x1b[H" + want
    assert R.stream(cur, 1, 1, viewport=(1, 0), default_fg=15, default_bg=0) == b"\x1b[1;1H" + both((255, 255, 255), (0, 0, 0)) + b" " + END


@pytest.mark.parametrize("second,escape", [((A2, B2), both(A2, B2)), ((A2, B1), fg_only(A2)), ((A1, B2), bg_only(B2)), ((A1, B1), b""),
                                           (((1, 2, 4), B1), fg_only((1, 2, 4)))])
def test_two_by_one_console_each_escape_branch_inside_a_run(second, escape):
    cur, shown = plane([[(A1, B1), second]]), plane([[FAR, FAR]])
    assert R.stream(cur, 2, 1) == b"\x1b[1;1H" + both(A1, B1) + UH + escape + UH + END
    got, info, new = R.delta(shown, cur, 2, 1)
    assert got == b"\x1b[1;1H" + both(A1, B1) + UH + escape + UH + END
    assert info == dict(keyframe=0, changed=2, emitted=2, runs=1) and (new == cur).all()


def test_two_by_one_console_reaches_the_bound_less_the_clear_prefix():
    cur, shown = plane([[((100, 200, 255), (101, 201, 254)), ((102, 202, 253), (103, 203, 252))]]), plane([[((0, 0, 0), (0, 0, 0))] * 2])
    assert R.bound(2, 1) == 7 + 4 + 6 + 78
    assert len(R.delta(shown, cur, 2, 1)[0]) == R.bound(2, 1) - 7
    assert len(R.stream(cur, 2, 1, clear=True)) == R.bound(2, 1)


def test_exhaustive_change_masks_of_one_row_stay_below_the_bound():
    w = 7
    shown = plane([[((0, 0, 0), (0, 0, 0))] * w])
    worst = 0
    for mask in itertools.product((0, 1), repeat=w):
        cur = plane([[((100 + x, 200, 255), (255, 199, 100 + x)) if m else ((0, 0, 0), (0, 0, 0)) for x, m in enumerate(mask)]])
        for gap in (0, 1, 3, 8):
            got, info, _ = R.delta(shown, cur, w, 1, gap=gap)
            assert len(got) <= R.bound(w, 1) - 7, (mask, gap)
            assert info["changed"] == sum(mask)
            worst = max(worst, len(got))
    assert worst == R.bound(w, 1) - 7          # (every cell changed: one run, every escape at its longest)


@pytest.mark.parametrize("v", [0, 9, 10, 99, 100, 255])
def test_digit_boundaries_of_a_channel(v):
    d = len(str(v))
    for ch in range(3):
        fg = [1, 1, 1]; fg[ch] = v
        s = R.stream(plane([[(tuple(fg), (2, 2, 2))]]), 1, 1)
        assert len(s) == 6 + (7 + 4 + d + 6 + 5 + 1) + 3 + 4
        assert R.Screen(1, 1).feed(s).grid[0][0] == (R.UPPER_HALF, tuple(fg), (2, 2, 2))
    assert R.Screen(1, 1).feed(R.stream(plane([[((v, v, v), (v, v, v))]]), 1, 1)).grid[0][0] == (R.UPPER_HALF, (v, v, v), (v, v, v))


def test_no_merge_across_a_row_end():
    base = ((7, 7, 7), (7, 7, 7))
    shown = plane([[base] * 4] * 3)
    cur = shown.copy()
    cur[2 * 0, 3, :3] = (9, 9, 9)          # (3, 0) and (0, 1): neighbours in raster order, two rows
    cur[2 * 1, 0, :3] = (8, 8, 8)
    got, info, _ = R.delta(shown, cur, 4, 3, gap=8)
    assert info == dict(keyframe=0, changed=2, emitted=3, runs=3)
    assert got == (b"\x1b[1;4H" + both((9, 9, 9), (7, 7, 7)) + UH + b"\x1b[2;1H" + both((8, 8, 8), (7, 7, 7)) + UH + b"\x1b[3;4H" + both((7, 7, 7), (7, 7, 7)) + UH + END)


def test_an_uncovered_last_cell():
    cur = plane([[(A1, B1), (A2, B2)]])
    pal = R.palette_rgb()
    got, info, new = R.delta(cur, cur, 3, 2, default_fg=2, default_bg=14)
    assert got == b"\x1b[2;3H" + both(pal[2], pal[14]) + b" " + END and info == dict(keyframe=0, changed=0, emitted=1, runs=1) and (new == cur).all()
    shown = cur.copy(); shown[0, 1, 0] = 99
    got, info, new = R.delta(shown, cur, 3, 2, default_fg=2, default_bg=14)
    assert got == b"\x1b[1;2H" + both(A2, B2) + UH + b"\x1b[2;3H" + both(pal[2], pal[14]) + b" " + END and info["runs"] == 2 and (new == cur).all()


def test_the_fourth_byte_is_ignored_and_the_new_shown_is_opaque():
    cur = plane([[(A1, B1), (A2, B2)]])
    other = cur.copy(); other[..., 3] = 7
    assert R.stream(other, 2, 1) == R.stream(cur, 2, 1)
    got, info, new = R.delta(other, cur, 2, 1)
    assert info["changed"] == 0 and (new[..., 3] == 255).all()


# ------------------------------------------------------------------------------------------------------------- the terminal
def _random_plane(rng, h, w, levels=4):
    return np.concatenate([(rng.integers(0, levels, (2 * h, w, 3)) * 60 + 5).astype(np.uint8), np.full((2 * h, w, 1), 255, np.uint8)], axis=-1)


@pytest.mark.parametrize("tol", [0, 1, 3, 255])
def test_a_delta_leaves_the_terminal_where_the_full_stream_does(tol):
    rng = np.random.default_rng(100 + tol)
    for case in range(60):
        fbW, fbH = int(rng.integers(1, 9)), int(rng.integers(1, 5))
        cw, ch = int(rng.integers(1, 11)), int(rng.integers(1, 6))
        vp = (int(rng.integers(-3, 4)), int(rng.integers(-2, 3)))
        gap = int(rng.integers(0, 9))
        frame = _random_plane(rng, fbH, fbW)
        screen, shown = R.Screen(cw, ch), None
        for k in range(5):
            got, info, shown = R.delta(shown, frame, cw, ch, vp, 3, 12, gap, tol)
            assert len(got) <= R.bound(cw, ch) and info["keyframe"] == int(k == 0)
            screen.feed(got)
            full = R.Screen(cw, ch).feed(R.stream(frame, cw, ch, vp, 3, 12))
            if tol == 0:
                assert screen.state() == full.state(), (case, k)
            assert R.within(screen, full, tol), (case, k)
            # what the restatement says the terminal shows is what the terminal shows
            assert screen.state() == R.Screen(cw, ch).feed(R.stream(shown, cw, ch, vp, 3, 12)).state(), (case, k)
            step = rng.integers(-2, 3, frame.shape) * (rng.random(frame.shape[:2] + (1,)) < 0.4)
            frame = np.clip(frame.astype(np.int64) + step, 0, 255).astype(np.uint8)
            frame[..., 3] = 255


def test_a_ramp_is_reemitted_on_every_third_frame():
    """a cell that rises by 1 per frame under tolerance 2: the comparison is against what the terminal shows, so it is rewritten when it is
    3 away from that - on every third frame - and never drifts further than 2; against the previous frame it would never be rewritten"""
    rest = ((50, 50, 50), (60, 60, 60))
    shown = None
    emitted_at = []
    screen = R.Screen(3, 1)
    for k in range(13):
        cur = plane([[((100 + k, 50, 50), (60, 60, 60)), rest, rest]])
        got, info, shown = R.delta(shown, cur, 3, 1, gap=0, tol=2)
        screen.feed(got)
        if k > 0 and info["changed"]:
            emitted_at.append(k)
            assert got.startswith(b"\x1b[1;1H" + both((100 + k, 50, 50), (60, 60, 60)))
        assert abs(screen.grid[0][0][1][0] - (100 + k)) <= 2 and tuple(shown[0, 0, :3]) == screen.grid[0][0][1]
    assert emitted_at == [3, 6, 9, 12]


# ------------------------------------------------------------------------------------------------------------- the library, host only
def _lib_bound(lib, cw, ch):
    n = C.c_size_t(0)
    return lib.ycge_ansi_rgb_stream_bound(cw, ch, C.byref(n)), n.value


def test_the_library_bound_equals_the_restatement(product_lib):
    for cw, ch in [(1, 1), (2, 1), (1, 9), (1, 10), (7, 99), (7, 100), (3, 1001), (81, 45), (641, 181), (1921, 541), (1, 99999), (10480, 10479)]:
        assert _lib_bound(product_lib, cw, ch) == (0, R.bound(cw, ch)), (cw, ch)
    for cw, ch in [(0, 1), (1, 0), (-1, 5), (5, -1)]:
        assert _lib_bound(product_lib, cw, ch)[0] == abi.YCGE_ERR_INVALID_ARG
    assert product_lib.ycge_ansi_rgb_stream_bound(1, 1, None) == abi.YCGE_ERR_INVALID_ARG
    assert _lib_bound(product_lib, 2 ** 31 - 1, 2 ** 31 - 1)[0] == abi.YCGE_ERR_INVALID_ARG          # (it does not fit a size_t)


def test_exports_are_declared_in_every_mirror(product_lib):
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    for name in EXPORTS:
        assert re.search(r"\bint " + name + r"\(", header) and not re.search(r"\b" + name + r"\s*\(", hooks), name
        assert name in abi.EXPORTED_SYMBOLS and hasattr(product_lib, name), name
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int " + name + r"\(", cs), name
    for name in abi.ANSI_RGB_HOOK_PROTOTYPES:
        assert re.search(r"\bint " + name + r"\(", hooks) and name not in header and hasattr(product_lib, name), name
    # the arguments of the forms they mirror; the deltas take `tolerance` behind merge_gap
    P = abi._PROTOTYPES
    assert P["ycge_render_frame_ansi_rgb"] == P["ycge_render_frame_ansi"] and P["ycge_video_blit_ansi_rgb"] == P["ycge_video_blit_ansi"]
    assert P["ycge_ansi_rgb_stream_bound"] == P["ycge_ansi_stream_bound"]
    for rgb, plain, at in (("ycge_render_frame_ansi_rgb_delta", "ycge_render_frame_ansi_delta", 9), ("ycge_video_blit_ansi_rgb_delta", "ycge_video_blit_ansi_delta", 13)):
        assert P[rgb][1] == P[plain][1][:at] + [C.c_int32] + P[plain][1][at:], rgb
        assert re.search(r"\bint " + rgb + r"\([^;]*int32_t merge_gap, int32_t tolerance,\s*int32_t keyframe", header), rgb
        assert re.search(rgb + r"\([^;]*int mergeGap,\s*int tolerance, int keyframe", cs), rgb
    assert "#define YCGE_ABI_VERSION 10" in header and abi.YCGE_ABI_VERSION == 10


def test_the_kernels_are_their_own_unit_and_the_exports_are_guarded():
    from yetanotherconsolegameengine_amd import build
    assert "ycge_ansi_rgb.hip" in build.SOURCES
    csrc = Path(abi.__file__).resolve().parent / "csrc"
    text = (csrc / "ycge_ansi.cpp").read_text()
    for n in EXPORTS + tuple(abi.ANSI_RGB_HOOK_PROTOTYPES):
        assert re.search(r"^int " + n + r"\([^{;]*?\)\ntry \{\n(.*?)\n\}\ncatch \(\.\.\.\) \{ return ycge_host::abi_catch\(", text, re.S | re.M), n


def test_the_wrappers_call_what_is_declared():
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    imports = {m.group(1): len([p for p in m.group(2).split(",") if p.strip()])
               for m in re.finditer(r"\[DllImport\(Lib\)\]\s*public static extern \w+ (ycge_\w+)\(([^)]*)\);", cs)}
    for fname, names in (("HipRaytraceWrapper.cs", ("ycge_render_frame_ansi_rgb", "ycge_render_frame_ansi_rgb_delta", "ycge_ansi_rgb_stream_bound")),
                         ("HipVideoWrapper.cs", ("ycge_video_blit_ansi_rgb", "ycge_video_blit_ansi_rgb_delta", "ycge_ansi_rgb_stream_bound"))):
        text = re.sub(r"//[^\n]*", "", (ROOT / "bindings" / "csharp" / fname).read_text())
        for name in names:
            m = re.search(r"Ycge\." + name + r"\(", text)
            assert m, (fname, name)
            i, depth, args, cur = m.end(), 1, 1, ""
            while depth:
                c = text[i]
                depth += c in "([{"
                depth -= c in ")]}"
                args += c == "," and depth == 1
                i += 1
            assert args == imports[name], (fname, name, args, imports[name])
    opts = (ROOT / "bindings" / "csharp" / "HipRaytraceWrapper.cs").read_text()
    assert re.search(r"public bool AnsiTrueColor\b[^;]*= false;", opts) and re.search(r"public int AnsiRgbTolerance\b[^;]*= 0;", opts)
