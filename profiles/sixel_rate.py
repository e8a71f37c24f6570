"""The sixel frames on the device (ycge_render_frame_sixel): what a synchronous frame costs against the 24-bit and the quadrant streams of
the same context geometry, what a stream carries with and without dither, and what the existing calls cost against the parent commit's
library.  One GPU, one process, one run.

    python profiles/sixel_rate.py [--parent-lib PATH --rounds 6 --frames-per-round 8]     -> profiles/sixel_rate.json

Config 4 in a 240 x 67 framebuffer at super_sample 8 - 1920 x 1072 pixels - under a 241 x 68 console.  The ANSI streams go into page-locked
memory of the library, the sixel stream into a pageable array of its bound's size (74 MB, of which a stream touches a few hundred KB); the
host clock around the calls, variants on contexts of their own, alternated round by round (the order reversed on odd rounds); per variant
the median, minimum and 99th percentile of the rounds.

(a) Frame time: `_sixel` (dither 0 and 1) against `_ansi_rgb` and `_ansi_quad`, the camera at rest, every context converged first.
(b) Bytes a frame of the sixel stream at dither 0 and 1, at rest (the mean over the frames behind the settling ones) and with the camera moving.
(c) With --parent-lib: `_ansi_rgb_delta` and plain ycge_render_frame through this library against the parent commit's, built elsewhere
    from the parent's sources and loaded beside it: two parent contexts and one product context, alternated.  The parent's own spread is
    max - min over the rounds of both its contexts; the claim held is "not slower by more than the parent differs from itself".
The new kernels' own times come from a kernel trace of `--trace-frames N` (this script run under the profiler, which writes them; the
figures are merged into the JSON by hand under "kernel_us").  Nothing here measures the terminal that consumes the bytes.
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
CONFIG, W, H, SS, GAP = 4, 240, 67, 8, 3
NEW_EXPORTS = ("ycge_sixel_stream_bound", "ycge_render_frame_pixels", "ycge_render_frame_sixel", "ycge_sixel_encode_host")


def renderer(lib=None):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, _, _, _, pose = scenes.config_scene(CONFIG)
    g = RaytraceRenderer(flatten(sc), W, H, pose.get("fov", 45.0), SS, lib=lib)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    g.pose = pose
    return g


def move(g, k):
    p = g.pose["pos"]
    g.SetCamera((p[0] + 0.02 * k, p[1], p[2] - 0.01 * k), g.pose["yaw"] + 0.01 * k, g.pose["pitch"])


def frame_fns(g, sixel=True):
    """call name -> a callable rendering one frame and returning the stream's length (the plain frame: 0)"""
    cw, ch = W + 1, H + 1
    cap = g.ansi_rgb_stream_bound(cw, ch, g.L)
    out = g._page_locked_zeros((cap,), np.uint8)[0]
    sdr = g._page_locked_zeros((H, W, 2, 3), np.float32)[0]
    p, n, info = out.ctypes.data_as(U8P), C.c_size_t(0), (C.c_uint32 * 4)()
    keep = [out, sdr]

    def rgb():
        g._check(g.L.ycge_render_frame_ansi_rgb(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
        return n.value

    def rgb_delta():
        g._check(g.L.ycge_render_frame_ansi_rgb_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, GAP, 0, 0, p, cap, C.byref(n), info, None, None))
        return n.value

    def quad():
        g._check(g.L.ycge_render_frame_ansi_quad(g.ctx, cw, ch, 0, 0, 7, 0, 0, 0, p, cap, C.byref(n), None, None))
        return n.value

    def plain():
        g._check(g.L.ycge_render_frame(g.ctx, sdr.ctypes.data_as(C.POINTER(C.c_float)), None))
        return 0
    fns = {"ansi rgb": rgb, "ansi rgb delta": rgb_delta, "ansi quad": quad, "render_frame": plain}
    if sixel:
        scap = g.sixel_stream_bound(W * SS, 2 * H * SS, g.L)
        sout = np.empty(scap, np.uint8)
        sp = sout.ctypes.data_as(U8P)
        keep.append(sout)

        def six(dither=0):
            g._check(g.L.ycge_render_frame_sixel(g.ctx, 0, 0, 0, dither, sp, scap, C.byref(n), None, None))
            return n.value
        fns["sixel"] = six
        fns["sixel dither"] = lambda: six(1)
    fns["_keep"] = keep
    return fns


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
            for _ in range(frames):
                size[v] = fn()
            per[v].append((time.perf_counter() - t0) * 1e3 / frames)
    return per, size


def frame_times(rounds, frames, settle):
    calls = ("ansi rgb", "ansi quad", "sixel", "sixel dither")
    ctxs = {c: renderer() for c in calls}
    fns = {c: frame_fns(g)[c] for c, g in ctxs.items()}          # (the callables hold their buffers)
    for c in calls:
        for _ in range(settle):
            fns[c]()
    per, size = timed(fns, rounds, frames)
    for g in ctxs.values():
        g.close()
    ms = {c: stats(v) for c, v in per.items()}
    return {"ms_per_frame": ms, "bytes_a_frame_at_rest": size, "rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle,
            "sixel_minus_rgb_ms": ms["sixel"]["median"] - ms["ansi rgb"]["median"], "sixel_minus_quad_ms": ms["sixel"]["median"] - ms["ansi quad"]["median"]}


def stream_bytes(settle, frames):
    res = {"frames_at_rest_before": settle, "frames_counted": frames, "variants": {}}
    for name in ("sixel", "sixel dither"):
        g = renderer()
        fn = frame_fns(g)[name]
        for _ in range(settle):
            fn()
        rest = [fn() for _ in range(frames)]
        moving = []
        for k in range(frames):
            move(g, k + 1)
            moving.append(fn())
        g.close()
        res["variants"][name] = {"at_rest_mean": float(np.mean(rest)), "at_rest_min": int(np.min(rest)), "at_rest_max": int(np.max(rest)),
                                 "moving_mean": float(np.mean(moving)), "moving_min": int(np.min(moving)), "moving_max": int(np.max(moving))}
        print(name, json.dumps(res["variants"][name]), flush=True)
    return res


def against_parent(parent_lib, rounds, frames, settle):
    from yetanotherconsolegameengine_amd import abi
    P = abi.bind(C.CDLL(str(parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n not in NEW_EXPORTS])
    assert not hasattr(P, NEW_EXPORTS[0]), "the parent's library is expected to lack the new exports"
    ctxs = {"parent A": renderer(P), "product": renderer(), "parent B": renderer(P)}
    fns = {k: frame_fns(g, sixel=False) for k, g in ctxs.items()}
    res = {"rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle, "calls": {}}
    for call in ("ansi rgb delta", "render_frame"):
        for f in fns.values():
            for _ in range(settle):
                f[call]()
        per, _ = timed({k: f[call] for k, f in fns.items()}, rounds, frames)
        parent = per["parent A"] + per["parent B"]
        spread = float(np.max(parent) - np.min(parent))
        diff = float(np.median(per["product"]) - np.median(parent))
        res["calls"][call] = {"ms_per_frame": {k: stats(v) for k, v in per.items()}, "parent_median_ms": float(np.median(parent)), "parent_spread_ms": spread,
                              "product_spread_ms": float(np.max(per["product"]) - np.min(per["product"])), "product_minus_parent_ms": diff,
                              "not_slower_by_more_than_the_parents_spread": bool(diff <= spread)}
        print("parent:", call, json.dumps(res["calls"][call]), flush=True)
    for g in ctxs.values():
        g.close()
    return res


def trace_frames(n):
    """n sixel frames at each dither, for a kernel trace taken from outside"""
    g = renderer()
    f = frame_fns(g)
    for _ in range(n):
        f["sixel"]()
    for _ in range(n):
        f["sixel dither"]()
    g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames-per-round", type=int, default=8)
    ap.add_argument("--settle", type=int, default=40)
    ap.add_argument("--byte-frames", type=int, default=20)
    ap.add_argument("--trace-frames", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sixel_rate.json"))
    a = ap.parse_args()
    if a.trace_frames:
        trace_frames(a.trace_frames)
        sys.exit(0)
    m = {"what": "the sixel frames on the device (ycge_render_frame_sixel) on one MI355X; profiles/sixel_rate.py", "config": CONFIG,
         "framebuffer": [W, H], "super_sample": SS, "pixels": [W * SS, 2 * H * SS], "console": [W + 1, H + 1],
         "kernel_us": "not yet run", "not_measured": "the terminal that consumes the bytes, and the C# wrappers (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    m["frame_times"] = frame_times(a.rounds, a.frames_per_round, a.settle)
    print("frame times", json.dumps(m["frame_times"]), flush=True)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
    m["stream_bytes"] = stream_bytes(a.settle, a.byte_frames)
    m["existing_calls_against_parent"] = against_parent(a.parent_lib, a.rounds, a.frames_per_round, a.settle) if a.parent_lib else "not measured"
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
