"""Device chexel colours, the parts that need no GPU: the restatement's known answers (tests/chexel_restatement.py), the library's
LinearToSrgb8 threshold tables (ycge_host_srgb_thresholds) held to the formula, and the new surface in every mirror."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import chexel_restatement as R
from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
NAN = float("nan")


def library_tables(lib):
    t32, t64 = np.zeros(255, F32), np.zeros(255, np.float64)
    assert lib.ycge_host_srgb_thresholds(t32.ctypes.data_as(C.c_void_p), t64.ctypes.data_as(C.c_void_p)) == 0
    return t32, t64


@pytest.fixture(scope="module")
def tables(product_lib):
    return library_tables(product_lib)


# ------------------------------------------------------------------------------------------------------------- known answers
def test_every_palette_entry_maps_to_itself():
    for i in range(16):
        assert R.color16(R.PALETTE16[i]) == i
    assert np.array_equal(R.color16_v(R.PALETTE16), np.arange(16))


@pytest.mark.parametrize("rgb,want", [
    ((0.25, 0.0, 0.0), 0),                  # black / DarkRed tie: the lower index
    ((0.0, 0.0, 0.25), 0),
    ((0.75, 0.0, 0.0), 4),                  # DarkRed / Red
    ((0.625, 0.625, 0.625), 7),             # Gray (7) / DarkGray (8): the lower index, the brighter colour
    ((0.875, 0.875, 0.875), 7),             # Gray / White
    ((0.25, 0.25, 0.25), 0),                # black / DarkGray
    ((NAN, NAN, NAN), 0), ((NAN, 1.0, 1.0), 0),
    ((-0.0, -0.0, -0.0), 0), ((-1.0, 2.0, -3.0), 10), ((5.0, 5.0, 5.0), 15), ((float("inf"), 0.0, float("-inf")), 12),
])
def test_color16_ties_and_edges(rgb, want):
    assert R.color16(rgb) == want
    assert R.color16_v(np.array([rgb], F32))[0] == want


def test_color16_midpoint_grid_picks_the_lowest_index_among_the_nearest():
    vals = [0.0, 0.25, 0.5, 0.625, 0.75, 0.875, 1.0]
    trip = np.array([(a, b, c) for a in vals for b in vals for c in vals], F32)
    d = ((trip[:, None, :] - R.PALETTE16[None, :, :]) ** 2).sum(-1, dtype=np.float64)      # exact for these values
    want = np.argmin(d, axis=1)                         # (the first minimum)
    assert np.array_equal(R.color16_v(trip), want)
    assert [R.color16(t) for t in trip] == list(want)


@pytest.mark.parametrize("rgb,want", [
    ((0.0, 0.0, 0.0), 16), ((1.0, 1.0, 1.0), 231), ((1.0, 0.0, 0.0), 196), ((0.0, 1.0, 0.0), 46), ((0.0, 0.0, 1.0), 21),
    ((NAN, 0.5, 0.5), 16 + 6 * 3 + 3),      # the NaN channel is byte 0; the luminance is NaN -> 0
    ((-2.0, 7.0, 0.5), 16 + 36 * 0 + 6 * 5 + 3),
    # a near gray: with s_graySrgb filled the ramp entry 232 + 12 (sRGB 128) would be nearest; the array is never filled, so the gray
    # candidate is measured to black and the cube entry 102 (135, 135, 135) wins
    ((0.2, 0.2, 0.2), 102),
])
def test_ansi256_known_answers(rgb, want):
    assert R.ansi256(rgb) == want
    assert R.ansi256_v(np.array([rgb], F32))[0] == want


def test_ansi256_the_gray_ramp_never_wins():
    """The quirk, taken to its end: for every cube level c(c - 2 v) <= 0, so the distance to the cube is never above the distance to
    black, and the gray candidate (to black, + 64) never wins - for every sRGB byte triple."""
    v = np.arange(256)
    lvl = (v >= 48).astype(int) + (v >= 114) + (v >= 154) + (v >= 194) + (v >= 234)
    cube = np.array(R.CUBE_SRGB)[lvl]
    assert np.all((v - cube) ** 2 <= v * v)


def test_linear_to_srgb8_known_answers():
    assert [R.linear_to_srgb8(x) for x in (0.0, -0.0, -1.0, 1.0, 2.0, NAN, float("inf"), float("-inf"), 0.0031308, 0.5)] == \
           [0, 0, 0, 255, 255, 0, 255, 0, 10, 188]
    # Math.Round is half to even: a value whose s * 255 is exactly k + 0.5 on the linear branch (12.92 c * 255 = 0.5 -> 0, = 1.5 -> 2)
    assert R.linear_to_srgb8(0.5 / (12.92 * 255.0)) in (0, 1)
    assert [round(0.5), round(1.5), round(2.5)] == [0, 2, 2]


def test_vectorised_restatement_equals_the_scalar_one():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.random(3000, dtype=np.float32) * 1.2 - 0.1, R.PALETTE16.ravel(),
                        np.array([NAN, -0.0, 0.0, 1.0, np.inf, -np.inf, 1e-40, 0.0031308, 0.25, 0.625, 0.875], F32)])
    x = x[: len(x) // 3 * 3].astype(F32).reshape(-1, 3)
    assert list(R.color16_v(x)) == [R.color16(t) for t in x]
    assert list(R.ansi256_v(x)) == [R.ansi256(t) for t in x]
    assert list(R.srgb8_v(x.ravel().astype(np.float64))) == [R.linear_to_srgb8(float(v)) for v in x.ravel()]


def test_encode_layouts():
    rng = np.random.default_rng(6)
    sdr = rng.random((3, 5, 2, 3), dtype=np.float32)
    c16, ansi, rgba = R.encode(sdr)
    assert c16.shape == (3, 5) and ansi.shape == (3, 5, 2) and rgba.shape == (6, 5, 4)
    for cy in range(3):
        for cx in range(5):
            top, bot = sdr[cy, cx, 0], sdr[cy, cx, 1]
            assert c16[cy, cx] == R.color16(top) | R.color16(bot) << 4
            assert tuple(ansi[cy, cx]) == (R.ansi256(top), R.ansi256(bot))
            assert tuple(rgba[2 * cy, cx]) == tuple(R.linear_to_srgb8(float(v)) for v in top) + (255,)
            assert tuple(rgba[2 * cy + 1, cx]) == tuple(R.linear_to_srgb8(float(v)) for v in bot) + (255,)


# ------------------------------------------------------------------------------------------------------------- the library's tables
def test_thresholds_are_the_formulas(tables):
    t32, t64 = tables
    a, b = R.thresholds_from_formula()
    assert np.array_equal(t32.view(np.uint32), a.view(np.uint32))
    assert np.array_equal(t64.view(np.uint64), b.view(np.uint64))
    assert np.all(np.diff(t32) > 0) and np.all(np.diff(t64) > 0) and t32[0] > 0 and t64[-1] <= 1.0


def test_f32_table_counts_the_formulas_byte(tables):
    """byte(x) = the number of thresholds <= x, on every binary32 within 2^16 ulps of each threshold and every 16th binary32 of [0, 1]"""
    t32, _ = tables
    tb = t32.view(np.uint32).astype(np.int64)
    near = (tb[:, None] + np.arange(-(1 << 16), 1 << 16)[None, :]).ravel()
    sweep = np.arange(0, 0x3F800001, 16, dtype=np.int64)
    for bits in (near, sweep):
        bits = np.unique(np.clip(bits, 0, 0x3F800000))
        for k in range(0, len(bits), 1 << 23):
            x = bits[k:k + (1 << 23)].astype(np.uint32).view(F32)
            assert np.array_equal(R.srgb8_v(x.astype(np.float64)), np.searchsorted(t32, x, side="right"))
    edge = np.array([NAN, -0.0, -1.0, 1.0, 1.5, np.inf, -np.inf], F32)
    with np.errstate(invalid="ignore"):
        counts = [(t32 <= v).sum() for v in edge]
    assert counts == [0, 0, 0, 255, 255, 255, 0]


def test_f64_table_counts_the_formulas_byte(tables):
    """... and the binary64 table at each threshold +- 1000 ulps and on 10 M random doubles (the luminance is a genuine double)"""
    _, t64 = tables
    tb = t64.view(np.uint64).astype(np.int64)
    near = np.unique((tb[:, None] + np.arange(-1000, 1001)[None, :]).ravel())
    rng = np.random.default_rng(64)
    for x in (near.astype(np.uint64).view(np.float64), rng.random(10_000_000)):
        assert np.array_equal(R.srgb8_v(x), np.searchsorted(t64, x, side="right"))


# ------------------------------------------------------------------------------------------------------------- the surface
def test_new_exports_in_every_mirror(product_lib):
    for name in ("ycge_render_frame_chexels", "ycge_render_frame_async_chexels"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(product_lib, name)
    assert abi.YCGE_ABI_VERSION == 10
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text()
    assert "ycge_host_srgb_thresholds(" in hooks and "ycge_test_encode_chexels(" in hooks


def test_csharp_wrapper_asks_the_device_for_color16():
    src = (ROOT / "bindings" / "csharp" / "HipRaytraceWrapper.cs").read_text()
    assert re.search(r"public bool DeviceChexelColors;", src)
    assert re.search(r"Ycge\.ycge_render_frame_chexels\(ctx, sdr, color16, null, null, null\)", src)
    assert re.search(r"Ycge\.ycge_render_frame_async_chexels\(ctx, sdrLate, color16Late, null, null\)", src)
    assert "new ChexelColor((ConsoleColor)(b & 15)" in src and "new ChexelColor((ConsoleColor)(b >> 4)" in src
