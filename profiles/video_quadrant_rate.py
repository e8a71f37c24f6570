"""Quadrant glyphs in Video mode on the device (ycge_video_blit_ansi_quad / _quad_delta): what a blit costs against the 24-bit video calls,
what the kernel alone costs against k_video_blit, what the delta carries, and what the existing call costs against the parent commit's
library.  One GPU, one process, one run.

    python profiles/video_quadrant_rate.py [--parent-lib PATH --rounds 8 --frames-per-round 10]     -> profiles/video_quadrant_rate.json

A 1920 x 1080 BGR source (seeded noise over a gradient, pageable, as a reader hands it over) into 240 x 67 and into 960 x 270 chexels at
super_sample 2, under a console of the framebuffer's size; every stream into page-locked memory of the library, the host clock around the
calls, variants on contexts of their own, alternated round by round (the order reversed on odd rounds), one warm-up call a round; per
variant the median, minimum and 99th percentile of the rounds.

(a) The call: `_ansi_quad` and `_ansi_quad_delta` against `_ansi_rgb` and `_ansi_rgb_delta`; the deltas for a still source and for one that
    changes every frame (two frames alternated), with the bytes a frame.
(b) The kernel alone: ycge_test_video_blit_quadrants against ycge_test_video_blit at the same shapes (upload, launch, synchronisation and
    the copies out: the hooks' whole cost, the quadrant one copying 12 more floats a chexel).
(c) With --parent-lib: ycge_video_blit_ansi_rgb through this library against the parent commit's, built elsewhere from the parent's
    sources and loaded beside it: two parent contexts and one product context, alternated.  The parent's own spread is its min-to-p99 over
    the rounds of both its contexts; the claim held is "not slower by more than the parent differs from itself".
Nothing here measures the reader that produces the frames or the terminal that consumes the bytes.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

U8P = C.POINTER(C.c_uint8)
SRC_W, SRC_H, BPP, SS, GAP = 1920, 1080, 3, 2, 3
SHAPES = ((240, 67), (960, 270))
NEW_EXPORTS = ("ycge_video_blit_quadrants", "ycge_video_blit_ansi_quad", "ycge_video_blit_ansi_quad_delta")


def sources():
    """two frames: a gradient under seeded noise, and the same with other noise (a source that changes every frame alternates them)"""
    y, x = np.mgrid[0:SRC_H, 0:SRC_W]
    base = np.stack([x * 255 // (SRC_W - 1), y * 255 // (SRC_H - 1), (x + y) * 255 // (SRC_W + SRC_H - 2)], axis=-1).astype(np.int64)
    out = []
    for seed in (1, 2):
        noise = np.random.default_rng(seed).integers(-24, 25, base.shape)
        out.append(np.ascontiguousarray(np.clip(base + noise, 0, 255).astype(np.uint8)))
    return out


def video(fw, fh, lib=None):
    from yetanotherconsolegameengine_amd.renderer import VideoRenderer
    return VideoRenderer(fw, fh, SS, lib=lib)


def call_fns(v, frames):
    """call name -> a callable blitting the next frame into page-locked memory and returning the stream's length"""
    fw, fh, r, L = v.fbW, v.fbH, v._r, v.L
    cap = r.ansi_rgb_stream_bound(fw, fh, L)
    out = r._page_locked_zeros((cap,), np.uint8)[0]
    p, n, info = out.ctypes.data_as(U8P), C.c_size_t(0), (C.c_uint32 * 4)()
    ptrs = [f.ctypes.data_as(U8P) for f in frames]
    k = [0]

    def nxt(moving):
        k[0] += 1
        return ptrs[k[0] % len(ptrs)] if moving else ptrs[0]

    def rgb(moving=False):
        r._check(L.ycge_video_blit_ansi_rgb(v.ctx, nxt(moving), SRC_W, SRC_H, BPP, fw, fh, 0, 0, 7, 0, 0, p, cap, C.byref(n), None))
        return n.value

    def rgb_delta(moving=False):
        r._check(L.ycge_video_blit_ansi_rgb_delta(v.ctx, nxt(moving), SRC_W, SRC_H, BPP, fw, fh, 0, 0, 7, 0, 0, GAP, 0, 0, p, cap, C.byref(n), info, None))
        return n.value

    def quad(moving=False):
        r._check(L.ycge_video_blit_ansi_quad(v.ctx, nxt(moving), SRC_W, SRC_H, BPP, fw, fh, 0, 0, 7, 0, 0, 0, p, cap, C.byref(n), None))
        return n.value

    def quad_delta(moving=False):
        r._check(L.ycge_video_blit_ansi_quad_delta(v.ctx, nxt(moving), SRC_W, SRC_H, BPP, fw, fh, 0, 0, 7, 0, 0, GAP, 0, 0, 0, p, cap, C.byref(n), info, None))
        return n.value

    def kernel():
        v.blit_probe(frames[0], fw, fh, SS)
        return 0

    def kernel_quad():
        v.blit_quadrants_probe(frames[0], fw, fh, SS)
        return 0
    return {"ansi rgb": rgb, "ansi quad": quad, "ansi rgb delta, still": rgb_delta, "ansi quad delta, still": quad_delta,
            "ansi rgb delta, changing": lambda: rgb_delta(True), "ansi quad delta, changing": lambda: quad_delta(True),
            "hook k_video_blit": kernel, "hook k_video_blit_quadrants": kernel_quad, "_keep": (out, frames)}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "p99": float(np.percentile(v, 99)), "max": float(np.max(v))}


def timed(variants, rounds, frames):
    names = list(variants)
    per, size = {v: [] for v in names}, {}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            fn = variants[v]
            fn()                          # (untimed: warms the variant's path after the others ran)
            t0 = time.perf_counter()
            total = 0
            for _ in range(frames):
                total += fn()
            per[v].append((time.perf_counter() - t0) * 1e3 / frames)
            size[v] = total / frames
    return per, size


def the_calls(fw, fh, frames, rounds, per_round):
    calls = ("ansi rgb", "ansi quad", "ansi rgb delta, still", "ansi quad delta, still", "ansi rgb delta, changing", "ansi quad delta, changing",
             "hook k_video_blit", "hook k_video_blit_quadrants")
    ctxs = {c: video(fw, fh) for c in calls}
    fns = {c: call_fns(v, frames)[c] for c, v in ctxs.items()}
    for c in calls:
        fns[c](); fns[c]()
    per, size = timed(fns, rounds, per_round)
    for v in ctxs.values():
        v.close()
    ms = {c: stats(v) for c, v in per.items()}
    ratio = lambda a, b: ms[a]["median"] / ms[b]["median"]
    return {"ms_per_call": ms, "bytes_a_frame": {c: size[c] for c in calls if c.startswith("ansi")}, "rounds": rounds, "calls_per_round": per_round,
            "quad_over_rgb": ratio("ansi quad", "ansi rgb"), "quad_delta_over_rgb_delta_still": ratio("ansi quad delta, still", "ansi rgb delta, still"),
            "quad_delta_over_rgb_delta_changing": ratio("ansi quad delta, changing", "ansi rgb delta, changing"),
            "hook_quadrants_over_hook_blit": ratio("hook k_video_blit_quadrants", "hook k_video_blit")}


def against_parent(fw, fh, frames, parent_lib, rounds, per_round):
    from yetanotherconsolegameengine_amd import abi
    P = abi.bind(C.CDLL(str(parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n not in NEW_EXPORTS])
    assert not hasattr(P, NEW_EXPORTS[0]), "the parent's library is expected to lack the new exports"
    ctxs = {"parent A": video(fw, fh, P), "product": video(fw, fh), "parent B": video(fw, fh, P)}
    fns = {k: call_fns(v, frames)["ansi rgb"] for k, v in ctxs.items()}
    for f in fns.values():
        f(); f()
    per, _ = timed(fns, rounds, per_round)
    parent = per["parent A"] + per["parent B"]
    spread = float(np.percentile(parent, 99) - np.min(parent))
    diff = float(np.median(per["product"]) - np.median(parent))
    for v in ctxs.values():
        v.close()
    return {"call": "ycge_video_blit_ansi_rgb", "ms_per_call": {k: stats(v) for k, v in per.items()}, "parent_median_ms": float(np.median(parent)),
            "parent_spread_min_to_p99_ms": spread, "product_spread_min_to_p99_ms": float(np.percentile(per["product"], 99) - np.min(per["product"])),
            "product_minus_parent_ms": diff, "not_slower_by_more_than_the_parents_spread": bool(diff <= spread), "rounds": rounds, "calls_per_round": per_round}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "video_quadrant_rate.json"))
    a = ap.parse_args()
    m = {"what": "quadrant glyphs in Video mode (ycge_video_blit_ansi_quad / _quad_delta) on one MI355X; profiles/video_quadrant_rate.py",
         "source": [SRC_W, SRC_H, BPP], "super_sample": SS, "merge_gap": GAP, "tolerance": 0, "min_contrast": 0,
         "not_measured": "the reader that produces the frames, the terminal that consumes the bytes, and the C# wrappers (never compiled here)", "shapes": {}}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    frames = sources()
    for fw, fh in SHAPES:
        r = the_calls(fw, fh, frames, a.rounds, a.frames_per_round)
        print(fw, fh, json.dumps(r), flush=True)
        r["existing_call_against_parent"] = against_parent(fw, fh, frames, a.parent_lib, a.rounds, a.frames_per_round) if a.parent_lib else "not measured"
        print(fw, fh, "parent:", json.dumps(r["existing_call_against_parent"]), flush=True)
        m["shapes"][f"{fw}x{fh}"] = r
        Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
