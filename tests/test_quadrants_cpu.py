"""The quadrant-glyph frames without a GPU: the restatement (tests/quadrant_restatement.py) pinned to the oracle's post stage in its half-cell
form, the properties of the integer fit, and the new exports and hooks in the built library."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

import oracle_binding as ob
import post_probe_inputs as ppi
import quadrant_restatement as Q

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
EXPORTS = ("ycge_render_frame_quadrants", "ycge_render_frame_ansi_quad", "ycge_render_frame_ansi_quad_delta")
HOOKS = ("ycge_test_quadrant_sdr", "ycge_test_quadrant_fit", "ycge_test_ansi_quad_stream", "ycge_test_ansi_quad_delta")


@pytest.mark.parametrize("fbw,fbh,ss", [(7, 3, 1), (5, 2, 2), (3, 2, 3)])
def test_half_cell_form_is_the_oracles_sdr(fbw, fbh, ss):
    """sub_cells(quadrants=False) of the oracle's own denoised buffer and effective exposure is the oracle's SDR array, bit for bit (NaN
    counted equal to NaN), on a tame draw and on draws that hold values <= 0, > 1, huge and not finite, from exposures 1, 0.1, 1.5"""
    W, H = fbw * ss, fbh * 2 * ss
    seen = dict(nonpositive=False, above_one=False, huge=False)
    for k, family in enumerate(("tame", "all_dark", "finite_isolated", "finite_rows", "nonfinite_isolated", "nonfinite_corner")):
        d = ppi.make_inputs(family, W, H, seed=11 + fbw)
        den, sdr, st = ob.post_probe(fbw, fbh, ss, d["hdr"], d["alb"], d["nrm"], d["dep"], d["sky"], 3, d["phi"], [1.0, 0.1, 1.5][k % 3])
        got = Q.sub_cells(den, fbw, fbh, ss, st["effective"], quadrants=False)
        assert got.shape == sdr.shape == (fbh, fbw, 2, 3) and got.dtype == f32
        assert ppi.nan_aware_mismatches(got, sdr) == 0, (family, fbw, fbh, ss)
        with np.errstate(invalid="ignore"):
            seen["nonpositive"] |= bool((den <= 0).any()); seen["above_one"] |= bool((den > 1).any()); seen["huge"] |= bool((np.abs(den) >= 1e30).any())
    assert all(seen.values()), seen


def test_quadrant_form_averages_the_right_samples():
    """each quadrant is its own ss / 2 x ss box: a buffer that is constant on every box maps to map_pixel of that constant, and the four boxes
    of a chexel tile its two half-cells"""
    fbw, fbh, ss = 3, 2, 4
    rng = np.random.default_rng(5)
    vals = (rng.integers(0, 128, (fbh, fbw, 4, 3)) / 64.0).astype(f32)          # (7 bits: every partial sum of 8 of them is exact)
    hdr = np.zeros((fbh * 2 * ss, fbw * ss, 3), f32)
    for cy, cx, k in itertools.product(range(fbh), range(fbw), range(4)):
        y0, x0 = (cy * 2 + k // 2) * ss, cx * ss + (k % 2) * (ss // 2)
        hdr[y0:y0 + ss, x0:x0 + ss // 2] = vals[cy, cx, k]
    got = Q.sub_cells(hdr, fbw, fbh, ss, 0.8)
    assert got.shape == (fbh, fbw, 4, 3)
    assert np.array_equal(got.view(np.uint32), Q.map_pixel(vals, 0.8).view(np.uint32))
    with pytest.raises(AssertionError):
        Q.sub_cells(np.zeros((12, 9, 3), f32), 3, 2, 3, 1.0)          # (an odd super_sample has no quadrants)


def _sq_error(Qb, m):
    """the squared error of the best two-colour approximation under mask m: real-valued means, exact for bytes in binary64"""
    F = [k for k in range(3) if m >> k & 1]
    B = [k for k in range(4) if k not in F]
    e = 0.0
    for ks in (F, B):
        if ks:
            a = np.asarray([Qb[k] for k in ks], np.float64)
            e += float(((a - a.mean(axis=0)) ** 2).sum())
    return e


def _cells():
    rng = np.random.default_rng(2025)
    drawn = rng.integers(0, 256, (400, 4, 3))
    near = np.clip(rng.integers(0, 256, (200, 1, 3)) + rng.integers(-3, 4, (200, 4, 3)), 0, 255)
    greys = np.array([[[v] * 3 for v in q] for q in itertools.product((0, 1, 2, 127, 128, 254, 255), repeat=4)])
    return np.concatenate([drawn, near, greys]).astype(np.int64)


def test_fit_minimises_the_squared_error_and_ties_go_down():
    cells = _cells()
    masks, fg, bg = Q.fit_bytes(cells, 0)
    for Qb, m, f, b in zip(cells, masks, fg, bg):
        errs = [_sq_error(Qb, c) for c in range(8)]
        assert abs(errs[int(m)] - min(errs)) <= 1e-6 * max(1.0, min(errs)), (Qb.tolist(), int(m), errs)
        scores = [Q.score(Qb, c) for c in range(8)]
        assert int(m) == scores.index(max(scores)) and max(scores) < 1 << 24          # the first of the largest; int32 with room
        assert (int(m), tuple(f), tuple(b)) == Q.fit_cell(Qb, 0)[:1] + tuple(tuple(int(v) for v in t) for t in Q.fit_cell(Qb, 0)[1:])
    # built ties: two equal quadrants against two others (complementary pairs score alike; the smaller mask wins)
    a, b = [10, 200, 30], [250, 20, 90]
    for Qb, want in (([a, a, b, b], 3), ([a, b, a, b], 5), ([b, a, a, b], 6), ([a, b, b, b], 1), ([b, b, b, a], 7), ([b, a, b, b], 2), ([b, b, a, b], 4)):
        assert Q.fit_cell(Qb)[0] == want, (Qb, Q.fit_cell(Qb))
    assert Q.fit_cell([a, a, b, b]) == (3, tuple(a), tuple(b)) and Q.fit_cell([b, b, b, a]) == (7, tuple(b), tuple(a))


def test_fit_symmetries_contrast_and_rounding():
    rng = np.random.default_rng(7)
    for _ in range(300):
        p, q = rng.integers(0, 256, 3).tolist(), rng.integers(0, 256, 3).tolist()
        assert Q.fit_cell([p, p, p, p]) == (0, tuple(p), tuple(p))                      # four equal quadrants
        assert Q.fit_cell([p, p, q, q])[0] in (0, 3)                                    # left = right
        assert Q.fit_cell([p, q, p, q])[0] in (0, 5)                                    # top = bottom
    cells = _cells()
    masks, fg, bg = Q.fit_bytes(cells, 255)
    assert not masks.any() and np.array_equal(fg, bg)                                   # min_contrast = 255: one colour everywhere
    assert np.array_equal(bg, (2 * cells.sum(axis=1) + 4) // 8)
    # the contrast threshold is inclusive, and compares against the rounded mean of all four
    assert Q.fit_cell([[10] * 3, [10] * 3, [10] * 3, [14] * 3], 3)[0] == 0 and Q.fit_cell([[10] * 3, [10] * 3, [10] * 3, [14] * 3], 2)[0] == 7
    # the means round half up: {1, 2} -> 2 (3/2), {0, 1, 1} -> 1 (2/3 rounds to 1), {0, 0, 1} -> 0, four of {0, 0, 1, 1} -> 1 (2/4)
    assert Q.fit_cell([[1] * 3, [2] * 3, [200] * 3, [200] * 3]) == (3, (2, 2, 2), (200, 200, 200))
    assert Q.fit_cell([[0] * 3, [1] * 3, [1] * 3, [200] * 3])[1:] == ((1, 1, 1), (200, 200, 200))
    assert Q.fit_cell([[0] * 3, [0] * 3, [1] * 3, [200] * 3])[1:] == ((0, 0, 0), (200, 200, 200))
    assert Q.fit_cell([[0] * 3, [0] * 3, [1] * 3, [1] * 3], 255) == (0, (1, 1, 1), (1, 1, 1))


def test_glyphs_are_the_eight_three_byte_blocks():
    assert len(Q.GLYPHS) == 8 and Q.GLYPHS[0] == Q.GLYPHS[3] == 0x2580 and len(set(Q.GLYPHS)) == 7
    for m, u in enumerate(Q.GLYPHS):
        assert (0x2596 <= u <= 0x259F or u in (0x2580, 0x258C)) and u != 0x20
        assert Q.LR.utf8(u) == chr(u).encode("utf-8") and len(Q.LR.utf8(u)) == 3
    # the glyph draws the mask: the Unicode names of the blocks, quadrant by quadrant {TL, TR, BL, BR}
    import unicodedata
    parts = {"UPPER LEFT": 1, "UPPER RIGHT": 2, "LOWER LEFT": 4, "LOWER RIGHT": 8}
    for m, u in enumerate(Q.GLYPHS):
        name = unicodedata.name(chr(u))
        drawn = {"UPPER HALF BLOCK": 3, "LEFT HALF BLOCK": 5}.get(name) or sum(v for k, v in parts.items() if k in name)
        assert drawn == (m if m else 3), (m, name)
    g, fg, bg, masks = Q.fit(np.zeros((5, 12), f32))
    assert g.dtype == np.uint16 and set(g.tolist()) == {0x2580} and not masks.any()
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    assert RaytraceRenderer.QUADRANT_GLYPHS == Q.GLYPHS


def test_fit_takes_the_encoders_bytes():
    """Q is LinearToSrgb8 of the clamped channel: NaN and negatives 0, above one 255"""
    cell = np.array([[np.nan, -1.0, 2.0], [0.0, 1.0, 0.5], [1e30, -0.0, 0.2], [0.0031308, 0.5, 1.0]], f32)
    b = Q.quadrant_bytes(cell)[0]
    assert b[0].tolist() == [0, 0, 255] and b[1].tolist() == [0, 255, 188] and b[2][0] == 255 and b[2][1] == 0
    g, fg, bg, m = Q.fit(cell.reshape(1, 12))
    assert (int(m[0]), tuple(fg[0]), tuple(bg[0])) == Q.fit_cell(b)


def test_composite_and_stream_of_a_one_cell_console():
    glyphs = np.array([[0x259B]], np.uint16)
    rgba = np.array([[[1, 2, 3, 255]], [[40, 50, 60, 255]]], np.uint8)
    assert Q.stream(glyphs, rgba, 1, 1) == b"\x1b[1;1H\x1b[38;2;1;2;3;48;2;40;50;60m" + "▛".encode() + b"\x1b[0m"
    s, info, shown = Q.delta(None, glyphs, rgba, 1, 1)
    assert s == Q.stream(glyphs, rgba, 1, 1) and info["keyframe"] == 1
    # only the glyph changes: the cell is emitted whatever the tolerance
    s, info, nxt = Q.delta(shown, np.array([[0x2596]], np.uint16), rgba, 1, 1, tol=255)
    assert info == dict(keyframe=0, changed=1, emitted=1, runs=1) and "▖".encode() in s and nxt[0][0, 0] == 0x2596
    # an uncovered cell is ' ' in the default colours
    g, c = Q.composite(glyphs, rgba, [], 0, 2, 1)
    assert g.tolist() == [[0x259B, 0x20]] and tuple(c[0, 1, :3]) == Q.R.palette_rgb()[7]


def test_exports_and_hooks_resolve(product_lib):
    """the three exports and the four hooks in the built library, the header, the hooks header and abi.py (the surface tests hold the
    prototypes to each other once the names are listed)"""
    import ctypes as C
    from yetanotherconsolegameengine_amd import abi, build
    header = (ROOT / "include" / "ycge.h").read_text(encoding="utf-8")
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert hasattr(product_lib, n) and n in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", header), n
    assert tuple(abi.QUADRANT_HOOK_PROTOTYPES) == HOOKS
    for n in HOOKS:
        assert hasattr(product_lib, n) and n not in abi.EXPORTED_SYMBOLS and re.search(r"\bint " + n + r"\(", hooks) and ("int " + n + "(") not in header, n
    assert "#define YCGE_ABI_VERSION 10" in header
    P = abi._PROTOTYPES
    rgb, quad = P["ycge_render_frame_ansi_rgb"][1], P["ycge_render_frame_ansi_quad"][1]
    assert quad == rgb[:8] + [C.c_int32] + rgb[8:]                                      # min_contrast behind clear_screen
    rgb, quad = P["ycge_render_frame_ansi_rgb_delta"][1], P["ycge_render_frame_ansi_quad_delta"][1]
    assert quad == rgb[:11] + [C.c_int32] + rgb[11:]                                    # ... behind keyframe
    # refusals that need no device: a NULL context
    assert product_lib.ycge_render_frame_quadrants(None, None, None, None, None, 0, None) == abi.YCGE_ERR_INVALID_ARG
    cs = (ROOT / "bindings" / "csharp" / "HipRaytraceWrapper.cs").read_text(encoding="utf-8")
    assert "QuadrantGlyphs" in cs and "QuadrantMinContrast" in cs and "Ycge.ycge_render_frame_ansi_quad_delta(" in cs and "Ycge.ycge_render_frame_ansi_quad(" in cs
