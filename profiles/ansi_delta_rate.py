"""The delta ANSI stream on the device (ycge_render_frame_ansi_delta): how many bytes a frame's stream takes per merge_gap, with the
camera at rest and with it moving every frame, and what a synchronous frame of the delta form costs against ycge_render_frame_ansi in
the same process.  One GPU, one process; the method of profiles/ansi_rate.py.

    python profiles/ansi_delta_rate.py [--frames 60 --rounds 8 --frames-per-round 20]     -> profiles/ansi_delta_rate.json

Config 4 at 1920 x 540 under a 1921 x 541 console.  Bytes: for each merge_gap 0..8 a fresh context renders frames 1..60, the first a
keyframe, once with the camera where the scene puts it and once with the camera stepped every frame; per frame the stream's length and
out_info {keyframe, changed, emitted, runs}.  The frames of a sequence are the same for every gap (the stream changes no frame state), so
the totals compare the gaps alone.  `best_merge_gap_at_rest` is the gap with the fewest total bytes over the resting sequence: the default
of HipRaytraceOptions.AnsiMergeGap.  Time: `_ansi_delta` (that gap) and `_ansi`, alternated round by round on one context that has
converged at rest, every destination page-locked memory of the library, the host clock around the call, the median of the rounds.
Nothing here measures the terminal that consumes the bytes.
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
FORMS = ("ansi delta", "ansi stream")


def renderer():
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(4)
    g = RaytraceRenderer(flatten(sc), w, h, pose.get("fov", 45.0), ss)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    return g, pose


def frame_fns(g):
    """{form: callable} rendering one frame into page-locked memory; the delta's returns (length, info), the stream's its length"""
    cw, ch = g.fbW + 1, g.fbH + 1
    cap = g.ansi_stream_bound(cw, ch, g.L)
    out = g._page_locked_zeros((cap,), np.uint8)[0]
    p, n, info = out.ctypes.data_as(U8P), C.c_size_t(0), (C.c_uint32 * 4)()

    def delta(gap, keyframe=0):
        g._check(g.L.ycge_render_frame_ansi_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, gap, keyframe, p, cap, C.byref(n), info, None, None))
        return n.value, [int(v) for v in info]

    def stream():
        g._check(g.L.ycge_render_frame_ansi(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
        return n.value
    return delta, stream


def sequence(gap: int, frames: int, moving: bool):
    g, pose = renderer()
    delta, _ = frame_fns(g)
    rows = []
    for k in range(frames):
        if moving:
            q = pose["pos"]
            g.SetCamera((q[0] + 0.02 * k, q[1], q[2] - 0.01 * k), pose["yaw"] + 0.01 * k, pose["pitch"])
        length, info = delta(gap)
        rows.append([length] + info)
    g.close()
    deltas = [r for r in rows if r[1] == 0]
    return {"frames": rows, "columns": ["bytes", "keyframe", "changed", "emitted", "runs"], "keyframe_bytes": rows[0][0],
            "delta_bytes_total": int(sum(r[0] for r in deltas)), "delta_bytes_median": float(np.median([r[0] for r in deltas])) if deltas else None,
            "delta_bytes_last": deltas[-1][0] if deltas else None}


def rate(gap: int, rounds: int, frames: int, settle: int):
    g, _ = renderer()
    delta, stream = frame_fns(g)
    fns = {"ansi delta": lambda: delta(gap), "ansi stream": stream}
    for _ in range(settle):              # the camera rests: TAA converges, the quantised cells freeze
        delta(gap)
    for f in FORMS:
        for _ in range(5):
            fns[f]()
    per = {f: [] for f in FORMS}
    for r in range(rounds):
        for f in (FORMS if r % 2 == 0 else tuple(reversed(FORMS))):
            if f == "ansi delta":
                delta(gap)               # (behind a round of full streams the first delta call is a keyframe: not timed)
            t0 = time.perf_counter()
            for _ in range(frames):
                fns[f]()
            per[f].append((time.perf_counter() - t0) * 1e3 / frames)
    res = {"merge_gap": gap, "rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle,
           "ms_per_frame": {f: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for f, v in per.items()}}
    res["delta_minus_stream_ms_median"] = res["ms_per_frame"]["ansi delta"]["median"] - res["ms_per_frame"]["ansi stream"]["median"]
    g.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ansi_delta_rate.json"))
    a = ap.parse_args()
    m = {"what": "the delta ANSI stream on the device (ycge_render_frame_ansi_delta) on one MI355X; profiles/ansi_delta_rate.py",
         "config": 4, "framebuffer": [1920, 540], "console": [1921, 541],
         "not_measured": "the terminal that consumes the bytes, and the C# presenter (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    for name, moving in (("at_rest", False), ("moving", True)):
        m[name] = {str(gap): sequence(gap, a.frames, moving) for gap in range(9)}
        print(name, {gap: v["delta_bytes_total"] for gap, v in m[name].items()}, flush=True)
    best = min(range(9), key=lambda gap: (m["at_rest"][str(gap)]["delta_bytes_total"], gap))
    m["best_merge_gap_at_rest"] = best
    m["rate"] = rate(best, a.rounds, a.frames_per_round, a.frames)
    print(json.dumps(m["rate"]), flush=True)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
