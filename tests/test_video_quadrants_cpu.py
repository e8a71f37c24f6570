"""Quadrant glyphs in Video mode without a GPU: the two forms of tests/video_quadrant_restatement.py against each other and against
video_restatement.blit, the conditions the inputs of tests/test_gpu_video_quadrants.py must meet (so that a green GPU test cannot be an empty
one), and the prototypes in the header, abi.py and the hooks header."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import quadrant_restatement as Q
import video_quadrant_inputs as I
import video_quadrant_restatement as VQ
import video_restatement as VR
from yetanotherconsolegameengine_amd import abi

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
EXPORTS = ("ycge_video_blit_quadrants", "ycge_video_blit_ansi_quad", "ycge_video_blit_ansi_quad_delta")
HOOK = "ycge_test_video_blit_quadrants"


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def restated():
    """the array form of every hook case on its noise frame, computed once: case -> (frame, sdr, quad_sdr)"""
    out = {}
    for c in I.HOOK_CASES:
        sw, sh, bpp, fw, fh, ss = c
        f = I.noise(sw, sh, bpp)
        out[c] = (f,) + VQ.blit_quadrants(f, sw, sh, bpp, fw, fh, ss)
    return out


def test_the_case_list_covers_the_table():
    cases = I.HOOK_CASES
    assert {c[3] for c in cases} >= {1, 63, 64, 65, 130} and {c[4] for c in cases} >= {1, 3} and {c[5] for c in cases} == {2, 4, 6}
    assert {c[2] for c in cases} == {3, 4}
    assert {(7, 5), (1, 1), (64, 6), (6, 64)} <= {c[:2] for c in cases}
    assert {(40, 30, 20, 5), (320, 200, 5, 2)} <= {c[:2] + c[3:5] for c in cases}
    s = I.SCALAR_CASES
    assert {c[5] for c in s} == {2, 4, 6} and {c[2] for c in s} == {3, 4} and {(7, 5), (1, 1), (40, 30), (320, 200), (64, 6), (6, 64)} <= {c[:2] for c in s}
    assert all(c in cases for c in I.CONTEXT_CASES)


@pytest.mark.parametrize("case", I.SCALAR_CASES, ids=I.case_id)
def test_scalar_and_array_forms_agree(restated, case):
    sw, sh, bpp, fw, fh, ss = case
    f, sdr, quad = restated[case]
    s_sdr, s_quad = VQ.blit_quadrants_scalar(f, sw, sh, bpp, fw, fh, ss)
    assert np.array_equal(bits(s_sdr), bits(sdr)) and np.array_equal(bits(s_quad), bits(quad))


def test_the_sdr_is_the_blits(restated):
    for (sw, sh, bpp, fw, fh, ss), (f, sdr, quad) in restated.items():
        assert np.array_equal(bits(sdr), bits(VR.blit(f, sw, sh, bpp, fw, fh, ss))), (sw, sh, bpp, fw, fh, ss)
        assert quad.shape == (fh, fw, 4, 3) and ((quad >= 0) & (quad <= 1)).all()


def test_at_ss_2_a_quadrant_is_its_two_samples_sum_times_a_half(restated):
    for c in [c for c in I.HOOK_CASES if c[5] == 2]:
        sw, sh, bpp, fw, fh, ss = c
        f, _, quad = restated[c]
        s = VQ.samples(f, sw, sh, bpp, fw, fh, 2)                           # (4 fbH, 2 fbW, 3)
        for k in range(4):
            col, row = k & 1, k >> 1
            a, b = s[2 * row::4, col::2], s[2 * row + 1::4, col::2]         # rows (2 cy + row) 2, + 1; column 2 cx + col
            want = (((f32(0) + a).astype(f32) + b).astype(f32) * f32(0.5)).astype(f32)
            want = np.minimum(np.maximum(want, f32(0)), f32(1))
            assert np.array_equal(bits(want), bits(quad[:, :, k])), (c, k)


def test_constant_frames_come_out_exact():
    """all 0 is 0.0 everywhere; all 255 is 1.0 everywhere on ONES_EXACT_CASES - an axis' normalised weights sum to 1 within an ulp only, so
    elsewhere the reference itself shows values an ulp or two below 1, and the GPU test holds those to the restatement instead"""
    below_one = 0
    for c in I.HOOK_CASES:
        sw, sh, bpp, fw, fh, ss = c
        sdr, quad = VQ.blit_quadrants(I.constant(sw, sh, bpp, 0), sw, sh, bpp, fw, fh, ss)
        assert not sdr.any() and not quad.any(), c
        sdr, quad = VQ.blit_quadrants(I.constant(sw, sh, bpp, 255), sw, sh, bpp, fw, fh, ss)
        if c in I.ONES_EXACT_CASES:
            assert (sdr == 1).all() and (quad == 1).all(), c
        else:
            below_one += int((quad < 1).sum())
            assert quad.min() > f32(0.999999), c
    assert all(c in I.HOOK_CASES for c in I.ONES_EXACT_CASES) and len(I.ONES_EXACT_CASES) >= 3 and below_one > 0


# ------------------------------------------------------------------------------------------------------------- what the GPU inputs must reach
def test_context_frames_reach_every_mask_and_flat_cells_under_min_contrast():
    for c in I.CONTEXT_CASES:
        sw, sh, bpp, fw, fh, ss = c
        frames = I.sequence(sw, sh, bpp)
        assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[2], frames[3]) and not np.array_equal(frames[1], frames[2])
        masks0 = np.zeros(8, np.int64)
        for f in (frames[0], frames[2]):
            _, quad = VQ.blit_quadrants(f, sw, sh, bpp, fw, fh, ss)
            masks0 += np.bincount(Q.fit(quad.reshape(-1, 12), 0)[3], minlength=8)
            _, fg, bg, m8 = Q.fit(quad.reshape(-1, 12), 8)
            flat = (m8 == 0) & (fg == bg).all(axis=1)
            assert ((m8 == 0) == flat).all()
            assert 0 < flat.sum() < fw * fh, (c, int(flat.sum()))          # some, not all
        assert (masks0 > 0).all(), (c, masks0.tolist())


def test_taps_are_clamped_at_each_frame_edge_and_the_last_pixel_is_a_three_byte_tap():
    edges = {"left": 0, "right": 0, "top": 0, "bottom": 0}
    last_pixel_bgr = 0
    for sw, sh, bpp, fw, fh, ss in I.HOOK_CASES:
        x0, _, y0, _, _ = VR.tables(sw, sh, fw, fh, ss)
        left, right, top, bottom = (x0 - 2 < 0).any(), (x0 + 3 > sw - 1).any(), (y0 - 2 < 0).any(), (y0 + 3 > sh - 1).any()
        for k, v in zip(edges, (left, right, top, bottom)):
            edges[k] += int(v)
        # the sample of the last hi-res row and column: its last tap is pixel (src_w - 1, src_h - 1), whose 32-bit load ends past the frame
        if bpp == 3 and min(max(int(x0[-1]) + 3, 0), sw - 1) == sw - 1 and min(max(int(y0[-1]) + 3, 0), sh - 1) == sh - 1:
            last_pixel_bgr += 1
    assert all(v > 0 for v in edges.values()), edges
    assert last_pixel_bgr > 0


def test_some_quadrant_halves_do_not_add_up_to_the_serial_sum(restated):
    """why the kernel carries the serial top / bottom sum beside the quadrant sums"""
    differ = 0
    for (sw, sh, bpp, fw, fh, ss), (f, _, _) in restated.items():
        serial, halves = VQ.sums(VQ.samples(f, sw, sh, bpp, fw, fh, ss), fw, fh, ss)
        differ += int((bits((halves[..., 0, :] + halves[..., 1, :]).astype(f32)) != bits(serial)).sum())
    assert differ > 0


# ------------------------------------------------------------------------------------------------------------- the mirrors
def test_the_header_abi_and_hooks_name_the_same_prototypes(product_lib):
    header = (ROOT / "include" / "ycge.h").read_text(encoding="utf-8")
    hooks = (ROOT / "include" / "ycge_hooks.h").read_text(encoding="utf-8")
    cs = (ROOT / "bindings" / "csharp" / "Ycge.cs").read_text(encoding="utf-8")
    for n in EXPORTS:
        assert hasattr(product_lib, n) and n in abi.EXPORTED_SYMBOLS, n
        assert re.search(r"\bint " + n + r"\(ycge_ctx \*ctx, const uint8_t \*frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,", header), n
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern int " + n + r"\(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel,", cs), n
    assert HOOK in abi.VIDEO_HOOK_PROTOTYPES and hasattr(product_lib, HOOK) and HOOK not in abi.EXPORTED_SYMBOLS
    assert re.search(r"\bint " + HOOK + r"\(", hooks) and HOOK not in header
    assert abi.VIDEO_HOOK_PROTOTYPES[HOOK][1] == abi.VIDEO_HOOK_PROTOTYPES["ycge_test_video_blit"][1] + [C.c_void_p]
    assert "#define YCGE_ABI_VERSION 10" in header and abi.YCGE_ABI_VERSION == 10
    P = abi._PROTOTYPES
    rgb, quad = P["ycge_video_blit_ansi_rgb"][1], P["ycge_video_blit_ansi_quad"][1]
    assert quad == rgb[:12] + [C.c_int32] + rgb[12:]                                    # min_contrast behind clear_screen
    rgb, quad = P["ycge_video_blit_ansi_rgb_delta"][1], P["ycge_video_blit_ansi_quad_delta"][1]
    assert quad == rgb[:15] + [C.c_int32] + rgb[15:]                                    # ... behind keyframe
    frame_form, video_form = P["ycge_render_frame_quadrants"][1], P["ycge_video_blit_quadrants"][1]
    assert video_form == P["ycge_video_blit"][1][:5] + frame_form[1:6]                  # the frame's five, then the planes call's destinations and min_contrast
    assert "the video blits" not in header[header.index("Not offered:"):][:200]
    # refusals that need no device: a NULL context
    assert product_lib.ycge_video_blit_quadrants(None, None, 1, 1, 3, None, None, None, None, 0) == abi.YCGE_ERR_INVALID_ARG
    wrapper = (ROOT / "bindings" / "csharp" / "HipVideoWrapper.cs").read_text(encoding="utf-8")
    assert "QuadrantGlyphs" in wrapper and "QuadrantMinContrast" in wrapper and "Ycge.ycge_video_blit_ansi_quad_delta(" in wrapper and "Ycge.ycge_video_blit_ansi_quad(" in wrapper
