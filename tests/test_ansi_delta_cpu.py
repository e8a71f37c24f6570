"""The delta ANSI stream without a GPU: known answers of its restatement (tests/ansi_delta_restatement.py), the terminal equivalence that
ties a delta to the full stream - a Screen that showed the previous frame shows, after the delta, what the full stream of the new frame
leaves, cursor and colours included - the length bound, and the surface of the new exports."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import ansi_delta_restatement as D
import ansi_stream_restatement as A
from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
UH = A.UPPER_HALF.encode("utf-8")
END = b"\x1b[0m"


def pairs(rows):
    return np.array(rows, np.uint8)


def both(fg, bg):
    return b"\x1b[38;5;%d;48;5;%dm" % (fg, bg)


# ------------------------------------------------------------------------------------------------------------- known answers
def test_one_by_one_console():
    cur = pairs([[(3, 4)]])
    want = b"\x1b[1;1H" + both(3, 4) + UH + END
    assert D.delta(cur, cur, 1, 1) == (want, dict(keyframe=0, changed=0, emitted=1, runs=1))          # the last cell, always
    assert D.delta(pairs([[(9, 9)]]), cur, 1, 1) == (want, dict(keyframe=0, changed=1, emitted=1, runs=1))
    assert D.delta(None, cur, 1, 1) == (A.stream(cur, 1, 1), dict(keyframe=1, changed=0, emitted=0, runs=0))


@pytest.mark.parametrize("second,escape", [((3, 4), both(3, 4)), ((3, 2), b"\x1b[38;5;3m"), ((1, 4), b"\x1b[48;5;4m"), ((1, 2), b"")])
def test_two_by_one_console_each_escape_branch_inside_a_run(second, escape):
    cur, prev = pairs([[(1, 2), second]]), pairs([[(200, 200), (201, 201)]])
    got, info = D.delta(prev, cur, 2, 1)
    assert got == b"\x1b[1;1H" + both(1, 2) + UH + escape + UH + END
    assert info == dict(keyframe=0, changed=2, emitted=2, runs=1)


def test_two_by_one_console_reaches_the_bound_less_the_clear_prefix():
    cur, prev = pairs([[(100, 200), (101, 201)]]), pairs([[(0, 0), (0, 0)]])
    assert len(D.delta(prev, cur, 2, 1)[0]) == A.bound(2, 1) - 7


def test_unchanged_frame_is_one_run_at_the_last_cell():
    rng = np.random.default_rng(5)
    cur = rng.integers(0, 256, (3, 5, 2)).astype(np.uint8)
    fg, bg = (int(v) for v in cur[2, 4])
    for gap in (0, 1, 8):
        assert D.delta(cur, cur.copy(), 5, 3, gap=gap) == (b"\x1b[3;5H" + both(fg, bg) + UH + END, dict(keyframe=0, changed=0, emitted=1, runs=1))


def test_no_merge_across_a_row_end():
    prev = np.full((3, 4, 2), 7, np.uint8)
    cur = prev.copy()
    cur[0, 3], cur[1, 0] = (10, 11), (12, 13)          # raster neighbours, in different rows
    got, info = D.delta(prev, cur, 4, 3, gap=8)
    assert got == b"\x1b[1;4H" + both(10, 11) + UH + b"\x1b[2;1H" + both(12, 13) + UH + b"\x1b[3;4H" + both(7, 7) + UH + END
    assert info == dict(keyframe=0, changed=2, emitted=3, runs=3)


@pytest.mark.parametrize("gap", range(9))
def test_gaps_of_g_cells_merge_and_of_g_plus_one_split(gap):
    w = 2 * gap + 8
    prev = np.full((2, w, 2), 7, np.uint8)
    merged, split = prev.copy(), prev.copy()
    merged[0, 1] = merged[0, 2 + gap] = (10, 11)           # `gap` unchanged cells between them
    split[0, 1] = split[0, 3 + gap] = (10, 11)             # gap + 1
    got, info = D.delta(prev, merged, w, 2, gap=gap)
    body = b"\x1b[1;2H" + both(10, 11) + UH + (both(7, 7) + UH + (gap - 1) * UH + both(10, 11) + UH if gap else UH)
    last = b"\x1b[2;%dH" % w + both(7, 7) + UH + END
    assert got == body + last and info == dict(keyframe=0, changed=2, emitted=gap + 3, runs=2)
    got, info = D.delta(prev, split, w, 2, gap=gap)
    assert got == b"\x1b[1;2H" + both(10, 11) + UH + b"\x1b[1;%dH" % (gap + 4) + both(10, 11) + UH + last
    assert info == dict(keyframe=0, changed=2, emitted=3, runs=3)


def test_uncovered_last_cell_is_a_space_in_the_default_colours():
    cur = np.full((2, 3, 2), 9, np.uint8)                  # the product's console: one column wider than the framebuffer
    pal = A.default_indices()
    assert D.delta(cur, cur, 4, 2, default_fg=15, default_bg=1)[0] == b"\x1b[2;4H" + both(pal[15], pal[1]) + b" " + END
    prev = cur.copy()
    prev[1, 2] = (1, 2)                                    # its left neighbour changed: one run, the space behind '▀'
    assert D.delta(prev, cur, 4, 2, default_fg=15, default_bg=1)[0] == b"\x1b[2;3H" + both(9, 9) + UH + both(pal[15], pal[1]) + b" " + END


# ------------------------------------------------------------------------------------------------------------- the terminal model
def test_screen_fails_on_bytes_no_stream_contains():
    for bad in (b"x", b"\x1b[1m", b"\x1b[3;", b"\x1b[38;5;1", b"\x1b[9;9H", b"\xe2\x96\x81"):
        with pytest.raises(AssertionError):
            D.Screen(4, 4).feed(b"\x1b[38;5;1;48;5;2m" + bad)
    with pytest.raises(AssertionError):
        D.Screen(2, 1).feed(b"\x1b[38;5;1;48;5;2m   ")          # a third character behind a pending wrap
    s = D.Screen(2, 2).feed(b"\x1b[2;1H\x1b[38;5;1;48;5;2m \x1b[48;5;3m" + UH + END)
    assert s.grid[1] == [(" ", 1, 2), (A.UPPER_HALF, 1, 3)] and s.cursor == (1, 1, True) and s.colours == (None, None)


def test_a_delta_leaves_the_terminal_where_the_full_stream_does():
    rng = np.random.default_rng(20261019)
    cases = 0
    for density in (0.0, 0.05, 0.3, 0.7, 1.0):
        for _ in range(80):
            fbW, fbH, cw, ch = (int(v) for v in (rng.integers(1, 14), rng.integers(1, 14), rng.integers(1, 16), rng.integers(1, 16)))
            vp = (int(rng.integers(-4, 6)), int(rng.integers(-4, 6)))
            if rng.random() < 0.1:
                vp = (int(rng.choice([-20, 20])), vp[1])          # fully off-screen
            gap, fg, bg, clear = int(rng.integers(0, 9)), int(rng.integers(0, 16)), int(rng.integers(0, 16)), bool(rng.integers(0, 2))
            prev = rng.integers(0, 4, (fbH, fbW, 2)).astype(np.uint8) * 85
            cur = np.where(rng.random((fbH, fbW, 1)) < density, rng.integers(0, 256, (fbH, fbW, 2)), prev).astype(np.uint8)
            stream, info = D.delta(prev, cur, cw, ch, vp, fg, bg, gap)
            assert info["keyframe"] == 0 and len(stream) <= A.bound(cw, ch)
            got = D.Screen(cw, ch).feed(A.stream(prev, cw, ch, vp, fg, bg, clear)).feed(stream)
            want = D.Screen(cw, ch).feed(A.stream(cur, cw, ch, vp, fg, bg, clear))
            assert got.state() == want.state(), (fbW, fbH, cw, ch, vp, gap, density)
            cases += 1
    assert cases == 400


# ------------------------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("row", [0, 9, 99], ids=["1-digit-row", "2-digit-row", "3-digit-row"])
def test_no_change_mask_of_a_small_console_exceeds_the_bound(row):
    """every change mask of row `row` (the last one, then one above the last) on consoles 1..7 wide, three-digit indices that differ
    between all neighbours, merge_gap 0, 1 and 3"""
    for cw, below in itertools.product(range(1, 8), (0, 1)):
        ch = row + 1 + below
        cur = np.zeros((ch, cw, 2), np.uint8)
        cur[..., 0], cur[..., 1] = 100 + np.arange(cw), 200 + np.arange(cw)
        bound, worst = A.bound(cw, ch), 0
        for mask in range(1 << cw):
            prev = cur.copy()
            prev[row, [x for x in range(cw) if mask >> x & 1]] = (0, 0)
            for gap in (0, 1, 3):
                worst = max(worst, len(D.delta(prev, cur, cw, ch, gap=gap)[0]))
        assert worst <= bound - 7, (cw, ch, worst, bound)


# ------------------------------------------------------------------------------------------------------------- the surface
def test_the_new_exports_are_declared_everywhere():
    header = (ROOT / "include" / "ycge.h").read_text()
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text()
    for name in ("ycge_render_frame_ansi_delta", "ycge_video_blit_ansi_delta"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in abi._PROTOTYPES and name in abi.EXPORTED_SYMBOLS
        assert re.search(r"\[DllImport\(Lib\)\] public static extern int %s\(" % name, cs), name
    assert re.search(r"^int ycge_test_ansi_delta\(", hooks, re.M) and "ycge_test_ansi_delta" not in header
    assert "ycge_test_ansi_delta" in abi.ANSI_DELTA_HOOK_PROTOTYPES
    assert len(abi._PROTOTYPES["ycge_render_frame_ansi_delta"][1]) == 16 and len(abi._PROTOTYPES["ycge_video_blit_ansi_delta"][1]) == 19
    assert "merge_gap" in header and "b - a - 1 <= G" in header


def test_the_kernels_live_in_their_own_unit_with_the_bound_proved():
    """the 256-colour unit instantiates the shared header, which carries the scheme of both colour forms once, the proof of the bound in
    its head; the delta stream has no unit of its own any more"""
    from yetanotherconsolegameengine_amd import build
    csrc = Path(abi.__file__).resolve().parent / "csrc"
    assert "ycge_ansi.hip" in build.SOURCES and "ycge_ansi_cells.hip.h" in build.HEADERS
    assert "ycge_ansi_delta.hip" not in build.SOURCES and not (csrc / "ycge_ansi_delta.hip").exists()
    src = (csrc / "ycge_ansi_cells.hip.h").read_text()
    assert "The bound." in src.split("#include")[0]
    for k in ("void k_delta_count(", "void k_scan(", "void k_delta_write("):
        assert k in src
    unit = (csrc / "ycge_ansi.hip").read_text()
    assert '#include "ycge_ansi_cells.hip.h"' in unit and "launch<Indexed>(" in unit


def test_the_default_merge_gap_is_the_measured_one():
    """profiles/ansi_delta_rate.json: the gap with the fewest total bytes over the resting sequence is the default everywhere"""
    import inspect
    import json
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer, VideoRenderer
    m = json.loads((ROOT / "profiles" / "ansi_delta_rate.json").read_text())
    totals = {int(g): v["delta_bytes_total"] for g, v in m["at_rest"].items()}
    best = min(sorted(totals), key=totals.get)
    assert sorted(totals) == list(range(9)) and best == m["best_merge_gap_at_rest"]
    for cls in (RaytraceRenderer, VideoRenderer):
        assert inspect.signature(cls.TryFlipAndBlitAnsiDelta).parameters["merge_gap"].default == best
    cs = (ROOT / "bindings" / "csharp" / "HipRaytraceWrapper.cs").read_text()
    assert re.search(r"public int AnsiMergeGap = %d;" % best, cs)
