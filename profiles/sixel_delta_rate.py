"""The delta sixel streams and sixel in Video mode on the device: stream bytes and call time of `_sixel_delta` against `_sixel`, for traced
frames (at rest and with the camera moving) and for video (a still and a changing source), plain and dithered - and what the existing calls
cost against the parent commit's library.  One GPU, one process, one run.

    python profiles/sixel_delta_rate.py [--parent-lib PATH --rounds 6 --frames-per-round 8]     -> profiles/sixel_delta_rate.json

The geometry of profiles/sixel_rate.json: config 4 in a 240 x 67 framebuffer at super_sample 8 - 1920 x 1072 pixels; the video source is a
1920 x 1080 BGR frame into the same pixels.  Streams go into a pageable array of the bound's size.  The host clock around the calls,
variants on contexts of their own, alternated round by round (profiles/sixel_rate.py's `timed`); per variant the median, minimum and 99th
percentile of the rounds.  With --parent-lib: `_sixel`, `ycge_video_blit_ansi_rgb` and plain ycge_render_frame through this library against
the parent commit's, two parent contexts and one product context alternated; unmoved means within the spread the parent's two contexts show.
The kernels' own times come from a kernel trace of `--trace-frames N` (this script run under the profiler; merged by hand under
"kernel_us").  Nothing here measures the terminal that consumes the bytes, nor the C# wrappers.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

import sixel_rate as R

U8P = C.POINTER(C.c_uint8)
W, H, SS = R.W, R.H, R.SS
SRC_W, SRC_H, BPP = 1920, 1080, 3
NEW_EXPORTS = ("ycge_video_blit_pixels", "ycge_video_blit_sixel", "ycge_render_frame_sixel_delta", "ycge_video_blit_sixel_delta", "ycge_sixel_encode_delta_host")


def source(k=0):
    """a drawn 1920 x 1080 BGR frame: gradients and a disc; k moves the disc (a changing source changes a region, as a film does)"""
    y, x = np.mgrid[0:SRC_H, 0:SRC_W]
    f = np.stack([(x * 255 // SRC_W), (y * 255 // SRC_H), ((x + y) * 255 // (SRC_W + SRC_H))], axis=-1).astype(np.uint8)
    cx, cy = 300 + 37 * k % 1300, 540 + 11 * k % 300
    f[(x - cx) ** 2 + (y - cy) ** 2 < 150 ** 2] = (30, 200, 240)
    return np.ascontiguousarray(f)


def sixel_fns(g):
    """name -> callable(dither) rendering one traced frame as a stream, returning its length"""
    cap = g.sixel_stream_bound(W * SS, 2 * H * SS, g.L)
    out, n, info = np.empty(cap, np.uint8), C.c_size_t(0), (C.c_uint32 * 4)()
    p = out.ctypes.data_as(U8P)

    def full(dither=0):
        g._check(g.L.ycge_render_frame_sixel(g.ctx, 0, 0, 0, dither, p, cap, C.byref(n), None, None))
        return n.value

    def delta(dither=0):
        g._check(g.L.ycge_render_frame_sixel_delta(g.ctx, 0, 0, 0, 0, dither, p, cap, C.byref(n), info, None, None))
        return n.value

    def video(frame, dither=0, delta=False):
        fp = frame.ctypes.data_as(U8P)
        if delta:
            g._check(g.L.ycge_video_blit_sixel_delta(g.ctx, fp, SRC_W, SRC_H, BPP, 0, 0, 0, 0, dither, p, cap, C.byref(n), info, None))
        else:
            g._check(g.L.ycge_video_blit_sixel(g.ctx, fp, SRC_W, SRC_H, BPP, 0, 0, 0, dither, p, cap, C.byref(n), None))
        return n.value
    return {"full": full, "delta": delta, "video": video, "info": info, "_keep": out}


def frames_section(rounds, frames, settle):
    res = {}
    for dither in (0, 1):
        ctxs = {"sixel": R.renderer(), "sixel delta": R.renderer()}
        f = {k: sixel_fns(g) for k, g in ctxs.items()}
        fns = {"sixel": lambda d=dither: f["sixel"]["full"](d), "sixel delta": lambda d=dither: f["sixel delta"]["delta"](d)}
        for fn in fns.values():
            for _ in range(settle):
                fn()
        per, size = R.timed(fns, rounds, frames)
        rest = {k: [fn() for _ in range(frames)] for k, fn in fns.items()}
        moving = {k: [] for k in fns}
        for j in range(frames):
            for k, g in ctxs.items():
                R.move(g, j + 1)
                moving[k].append(fns[k]())
        for g in ctxs.values():
            g.close()
        res["dither %d" % dither] = {"ms_per_frame_at_rest": {k: R.stats(v) for k, v in per.items()},
                                     "bytes_at_rest": {k: {"mean": float(np.mean(v)), "min": int(np.min(v)), "max": int(np.max(v))} for k, v in rest.items()},
                                     "bytes_moving": {k: {"mean": float(np.mean(v)), "min": int(np.min(v)), "max": int(np.max(v))} for k, v in moving.items()}}
        print("frames dither", dither, json.dumps(res["dither %d" % dither]), flush=True)
    return res


def video_section(rounds, frames):
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    still = source(0)
    changing = [source(k) for k in range(1, 5)]
    res = {}
    for dither in (0, 1):
        ctxs = {k: RaytraceRenderer(None, W, H, 45.0, SS) for k in ("sixel still", "delta still", "sixel changing", "delta changing")}
        f = {k: sixel_fns(g) for k, g in ctxs.items()}
        turn = {"n": 0}

        def nxt():
            turn["n"] += 1
            return changing[turn["n"] % len(changing)]
        fns = {"sixel still": lambda d=dither: f["sixel still"]["video"](still, d), "delta still": lambda d=dither: f["delta still"]["video"](still, d, True),
               "sixel changing": lambda d=dither: f["sixel changing"]["video"](nxt(), d), "delta changing": lambda d=dither: f["delta changing"]["video"](nxt(), d, True)}
        for fn in fns.values():
            fn(); fn()
        per, _ = R.timed(fns, rounds, frames)
        sizes = {k: [fn() for _ in range(8)] for k, fn in fns.items()}
        for g in ctxs.values():
            g.close()
        res["dither %d" % dither] = {"ms_per_call": {k: R.stats(v) for k, v in per.items()},
                                     "bytes": {k: {"mean": float(np.mean(v)), "min": int(np.min(v)), "max": int(np.max(v))} for k, v in sizes.items()}}
        print("video dither", dither, json.dumps(res["dither %d" % dither]), flush=True)
    return res


def against_parent(parent_lib, rounds, frames, settle):
    from yetanotherconsolegameengine_amd import abi
    P = abi.bind(C.CDLL(str(parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n not in NEW_EXPORTS])
    assert not hasattr(P, NEW_EXPORTS[0]), "the parent's library is expected to lack the new exports"
    ctxs = {"parent A": R.renderer(P), "product": R.renderer(), "parent B": R.renderer(P)}
    still = source(0)
    fns = {}
    for k, g in ctxs.items():
        base = R.frame_fns(g, sixel=True)
        cw, ch = W + 1, H + 1
        cap = g.ansi_rgb_stream_bound(cw, ch, g.L)
        out, n = np.empty(cap, np.uint8), C.c_size_t(0)

        def video_rgb(g=g, out=out, n=n, cap=cap):
            g._check(g.L.ycge_video_blit_ansi_rgb(g.ctx, still.ctypes.data_as(U8P), SRC_W, SRC_H, BPP, cw, ch, 0, 0, 7, 0, 0, out.ctypes.data_as(U8P), cap, C.byref(n), None))
            return n.value
        fns[k] = {"sixel": base["sixel"], "render_frame": base["render_frame"], "video ansi rgb": video_rgb, "_keep": (base, out)}
    res = {"rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle, "calls": {}}
    for call in ("sixel", "video ansi rgb", "render_frame"):
        for f in fns.values():
            for _ in range(settle if call != "video ansi rgb" else 2):
                f[call]()
        per, _ = R.timed({k: f[call] for k, f in fns.items()}, rounds, frames)
        parent = per["parent A"] + per["parent B"]
        spread = float(np.max(parent) - np.min(parent))
        diff = float(np.median(per["product"]) - np.median(parent))
        res["calls"][call] = {"ms_per_frame": {k: R.stats(v) for k, v in per.items()}, "parent_median_ms": float(np.median(parent)), "parent_spread_ms": spread,
                              "product_minus_parent_ms": diff, "not_slower_by_more_than_the_parents_spread": bool(diff <= spread)}
        print("parent:", call, json.dumps(res["calls"][call]), flush=True)
    for g in ctxs.values():
        g.close()
    return res


def trace_frames(n):
    """n frames of each new form, for a kernel trace taken from outside"""
    g = R.renderer()
    f = sixel_fns(g)
    frames = [source(k) for k in range(2)]
    for d in (0, 1):
        for k in range(n):
            R.move(g, k)
            f["delta"](d)
        for k in range(n):
            f["video"](frames[k & 1], d, True)
    g.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames-per-round", type=int, default=8)
    ap.add_argument("--settle", type=int, default=40)
    ap.add_argument("--trace-frames", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sixel_delta_rate.json"))
    a = ap.parse_args()
    if a.trace_frames:
        trace_frames(a.trace_frames)
        sys.exit(0)
    m = {"what": "delta sixel streams and sixel in Video mode on one MI355X; profiles/sixel_delta_rate.py", "config": R.CONFIG, "framebuffer": [W, H],
         "super_sample": SS, "pixels": [W * SS, 2 * H * SS], "video_source": [SRC_W, SRC_H, BPP], "kernel_us": "not yet run",
         "not_measured": "the terminal that consumes the bytes, and the C# wrappers (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    m["frames"] = frames_section(a.rounds, a.frames_per_round, a.settle)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
    m["video"] = video_section(a.rounds, a.frames_per_round)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
    m["existing_calls_against_parent"] = against_parent(a.parent_lib, a.rounds, a.frames_per_round, a.settle) if a.parent_lib else "not measured"
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
