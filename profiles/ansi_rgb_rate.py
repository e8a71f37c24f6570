"""The 24-bit colour ANSI streams on the device (ycge_render_frame_ansi_rgb, ycge_render_frame_ansi_rgb_delta): how many bytes a frame's
stream takes per tolerance and per merge_gap, with the camera at rest and with it moving every frame, and what a synchronous frame of each
form costs against the 256-colour forms in the same process.  One GPU, one process; the method of profiles/ansi_delta_rate.py.

    python profiles/ansi_rgb_rate.py [--frames 60 --rounds 8 --frames-per-round 20 --parent-lib PATH]     -> profiles/ansi_rgb_rate.json

Config 4 at 1920 x 540 under a 1921 x 541 console.  Bytes: for each tolerance in {0, 1, 2, 4, 8} at the default merge_gap 3, and for each
merge_gap in {0, 1, 3, 8} at tolerance 2, a fresh context renders frames 1..60, the first a keyframe, once with the camera where the
scene puts it and once with the camera stepped every frame; per sequence the keyframe's length, the deltas' total, median and last
length and the last frame's out_info.  The 256-colour delta at merge_gap 3 runs the same two sequences: the yardstick of "the order of
17 KB at rest".  Time: `_ansi_rgb`, `_ansi_rgb_delta` (tolerance 0 and 2), `_ansi` and `_ansi_delta`, alternated round by round on ONE
context that has converged at rest, every destination page-locked memory of the library, the host clock around the call, the median of
the rounds.  The check: the median of `_ansi_rgb_delta` lies within max - min of `_ansi_delta`'s rounds of `_ansi_delta`'s median, plus
the copy time of the extra bytes priced from the two full streams ((ms_rgb - ms_256) / (bytes_rgb - bytes_256): kernels' stores and the
copy together, so an upper price).  With --parent-lib, the parent commit's library (built elsewhere from the parent's sources) is loaded
beside the product's: two legs of the parent and one of the product run the five forms, alternated round by round (`rate_against_parent`,
parent_check below).  Nothing here measures the terminal that consumes the bytes.
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
TOLERANCES, GAPS, DEFAULT_GAP, GAP_TOLERANCE = (0, 1, 2, 4, 8), (0, 1, 3, 8), 3, 2
FORMS = ("ansi rgb delta T=0", "ansi rgb delta T=2", "ansi delta", "ansi rgb stream", "ansi stream")


def renderer(lib=None):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(4)
    g = RaytraceRenderer(flatten(sc), w, h, pose.get("fov", 45.0), ss, lib=lib)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    return g, pose


def frame_fns(g):
    """callables rendering one frame into page-locked memory: the deltas return (length, info), the full streams their length"""
    cw, ch = g.fbW + 1, g.fbH + 1
    cap = g.ansi_rgb_stream_bound(cw, ch, g.L)
    out = g._page_locked_zeros((cap,), np.uint8)[0]
    p, n, info = out.ctypes.data_as(U8P), C.c_size_t(0), (C.c_uint32 * 4)()

    def rgb_delta(gap, tol):
        g._check(g.L.ycge_render_frame_ansi_rgb_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, gap, tol, 0, p, cap, C.byref(n), info, None, None))
        return n.value, [int(v) for v in info]

    def delta(gap):
        g._check(g.L.ycge_render_frame_ansi_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, gap, 0, p, cap, C.byref(n), info, None, None))
        return n.value, [int(v) for v in info]

    def rgb_stream():
        g._check(g.L.ycge_render_frame_ansi_rgb(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
        return n.value

    def stream():
        g._check(g.L.ycge_render_frame_ansi(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
        return n.value
    return rgb_delta, delta, rgb_stream, stream


def sequence(frames: int, moving: bool, gap: int, tol):
    """tol None: the 256-colour delta"""
    g, pose = renderer()
    rgb_delta, delta, _, _ = frame_fns(g)
    rows = []
    for k in range(frames):
        if moving:
            q = pose["pos"]
            g.SetCamera((q[0] + 0.02 * k, q[1], q[2] - 0.01 * k), pose["yaw"] + 0.01 * k, pose["pitch"])
        length, info = delta(gap) if tol is None else rgb_delta(gap, tol)
        rows.append([length] + info)
    g.close()
    deltas = [r for r in rows if r[1] == 0]
    return {"merge_gap": gap, "tolerance": tol, "keyframe_bytes": rows[0][0], "delta_frames": len(deltas),
            "delta_bytes_total": int(sum(r[0] for r in deltas)), "delta_bytes_median": float(np.median([r[0] for r in deltas])),
            "delta_bytes_last": deltas[-1][0], "last_frame": dict(zip(("bytes", "keyframe", "changed", "emitted", "runs"), rows[-1]))}


def form_fns(g, settle: int):
    """the five forms on g, converged at rest"""
    rgb_delta, delta, rgb_stream, stream = frame_fns(g)
    for _ in range(settle):              # the camera rests: TAA converges
        delta(DEFAULT_GAP)
    return {"ansi rgb delta T=0": lambda: rgb_delta(DEFAULT_GAP, 0), "ansi rgb delta T=2": lambda: rgb_delta(DEFAULT_GAP, 2), "ansi delta": lambda: delta(DEFAULT_GAP),
            "ansi rgb stream": rgb_stream, "ansi stream": stream}


def parent_check(per):
    """per: (leg, form) -> [ms a frame of each round], the legs "parent A", "branch", "parent B" (two of the parent's, as
    profiles/ansi_layers_rate.py has them: what differs between two legs of ONE build is part of the noise) -> form -> the parent's median
    and spread (max - min) over the rounds of both its legs, each leg's median, and whether the branch's lies at or below the parent's
    median plus its spread.  Every round of a leg runs on a context of its own, the only one alive: a context's place among the live
    contexts of a process changes its period whichever library made it (of three, the second ran its frames in flight 0.25 ms slower
    and the third its synchronous frames 0.2 ms slower)"""
    res = {}
    for f in dict.fromkeys(f for _, f in per):
        p, b = per[("parent A", f)] + per[("parent B", f)], per[("branch", f)]
        res[f] = {"parent_median_ms": float(np.median(p)), "parent_spread_ms": float(np.max(p) - np.min(p)), "branch_median_ms": float(np.median(b)),
                  "branch_spread_ms": float(np.max(b) - np.min(b)), "parent_A_median_ms": float(np.median(per[("parent A", f)])),
                  "parent_B_median_ms": float(np.median(per[("parent B", f)]))}
        res[f]["within_allowance"] = bool(res[f]["branch_median_ms"] <= res[f]["parent_median_ms"] + res[f]["parent_spread_ms"])
    return res


def rate_against_parent(parent_lib, rounds: int, frames: int, settle: int):
    from yetanotherconsolegameengine_amd import abi
    P = abi.load_library(parent_lib)
    libs = {"parent A": P, "branch": None, "parent B": P}
    per = {(b, f): [] for b in libs for f in FORMS}
    for r in range(rounds):
        for b in (list(libs) if r % 2 == 0 else list(libs)[::-1]):
            g, _ = renderer(libs[b])
            fns = form_fns(g, settle)
            for f in FORMS:
                for _ in range(5):
                    fns[f]()
            for f in FORMS:
                if "delta" in f:
                    fns[f]()             # (behind another form the first delta call is a keyframe: not timed)
                t0 = time.perf_counter()
                for _ in range(frames):
                    fns[f]()
                per[(b, f)].append((time.perf_counter() - t0) * 1e3 / frames)
            g.close()
    return dict(parent_check(per), rounds=rounds, frames_per_round=frames, frames_at_rest_before=settle)


def rate(rounds: int, frames: int, settle: int):
    g, _ = renderer()
    fns = form_fns(g, settle)
    for f in FORMS:
        for _ in range(5):
            fns[f]()
    per, size = {f: [] for f in FORMS}, {}
    for r in range(rounds):
        for f in (FORMS if r % 2 == 0 else tuple(reversed(FORMS))):
            if "delta" in f:
                fns[f]()                 # (behind another form the first delta call is a keyframe: not timed)
            t0 = time.perf_counter()
            for _ in range(frames):
                last = fns[f]()
            per[f].append((time.perf_counter() - t0) * 1e3 / frames)
            size[f] = last[0] if isinstance(last, tuple) else last
    ms = {f: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for f, v in per.items()}
    res = {"merge_gap": DEFAULT_GAP, "rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle, "ms_per_frame": ms, "bytes_last_frame": size}
    ms_per_byte = (ms["ansi rgb stream"]["median"] - ms["ansi stream"]["median"]) / max(1, size["ansi rgb stream"] - size["ansi stream"])
    spread = ms["ansi delta"]["max"] - ms["ansi delta"]["min"]
    res["stream_ms_per_extra_byte"] = ms_per_byte
    res["ansi_delta_spread_ms"] = spread
    for f in FORMS[:2]:
        extra = max(0, size[f] - size["ansi delta"])
        over = ms[f]["median"] - ms["ansi delta"]["median"]
        res[f] = {"minus_ansi_delta_ms_median": over, "extra_bytes": extra, "allowance_ms": spread + extra * max(0.0, ms_per_byte),
                  "within_allowance": bool(over <= spread + extra * max(0.0, ms_per_byte))}
    g.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="the parent commit's library, measured beside the product's")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ansi_rgb_rate.json"))
    a = ap.parse_args()
    m = {"what": "the 24-bit colour ANSI streams on the device (ycge_render_frame_ansi_rgb / _rgb_delta) on one MI355X; profiles/ansi_rgb_rate.py",
         "config": 4, "framebuffer": [1920, 540], "console": [1921, 541],
         "not_measured": "the terminal that consumes the bytes, and the C# presenter (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    for name, moving in (("at_rest", False), ("moving", True)):
        m[name] = {"by_tolerance": {str(t): sequence(a.frames, moving, DEFAULT_GAP, t) for t in TOLERANCES},
                   "by_merge_gap": {str(gap): sequence(a.frames, moving, gap, GAP_TOLERANCE) for gap in GAPS},
                   "ansi_delta_256": sequence(a.frames, moving, DEFAULT_GAP, None)}
        print(name, "median delta bytes by tolerance", {t: v["delta_bytes_median"] for t, v in m[name]["by_tolerance"].items()},
              "by merge_gap", {gap: v["delta_bytes_median"] for gap, v in m[name]["by_merge_gap"].items()},
              "256-colour", m[name]["ansi_delta_256"]["delta_bytes_median"], flush=True)
    m["rate"] = rate(a.rounds, a.frames_per_round, a.frames)
    print(json.dumps(m["rate"]), flush=True)
    if a.parent_lib:
        m["rate_against_parent"] = rate_against_parent(a.parent_lib, a.rounds, a.frames_per_round, a.frames)
        print(json.dumps(m["rate_against_parent"]), flush=True)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
