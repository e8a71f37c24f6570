"""The ANSI escape stream on the device (ycge_render_frame_ansi): what a synchronous frame costs when the host reads back the bytes
ANSITerminalRenderer.Render() writes, against the SDR frame and the ANSI-pairs frame, and how long the stream is.  One GPU, one process.

    python profiles/ansi_rate.py --part rate   --out DIR [--rounds R --frames K]   ms/frame of each form, config 4 -> DIR/rate.json
    python profiles/ansi_rate.py --part bytes  --out DIR                           stream bytes per frame, configs 1-5 -> DIR/bytes.json
    python profiles/ansi_rate.py --part kernel --out DIR                           a short run of the stream form (for rocprofv3)
    python profiles/ansi_rate.py --part merge  --out DIR [--kernel-stats FILE] [--bench-logs LOG ...]   -> profiles/ansi_rate.json

Forms, alternated round by round: `ansi stream` is ycge_render_frame_ansi for a console one cell wider and taller than the framebuffer
(config 4: 1921 x 541 over 1920 x 540) - the stream alone, no SDR; `sdr` is ycge_render_frame(sdr), today's frame; `chexels ansi` is
ycge_render_frame_chexels with the ANSI pairs alone.  Every destination is page-locked memory of the library.  A frame's time is the
host clock around the call, which returns with the frame in the caller's memory.  The kernels' times come from a separate
`rocprofv3 --kernel-trace --stats -- python profiles/ansi_rate.py --part kernel` run, whose rocpd database (or kernel_stats.csv) the
merge reads.  Nothing here measures the .NET presenter: the host time ANSITerminalRenderer.Render() spends is not known.
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

FORMS = ("ansi stream", "sdr", "chexels ansi")
U8P = C.POINTER(C.c_uint8)


def renderer(n):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(n)
    g = RaytraceRenderer(flatten(sc), w, h, pose.get("fov", 45.0), ss)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    return g


def frame_fn(g, form):
    """a callable that renders one frame of `form` into page-locked memory of the library; for the stream, its length"""
    cw, ch = g.fbW + 1, g.fbH + 1
    if form == "ansi stream":
        cap = g.ansi_stream_bound(cw, ch, g.L)
        out = g._page_locked_zeros((cap,), np.uint8)[0]
        n = C.c_size_t(0)
        p = out.ctypes.data_as(U8P)

        def fn():
            g._check(g.L.ycge_render_frame_ansi(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
            return n.value
        return fn
    shapes = g.chexel_shapes()
    if form == "sdr":
        a = g._page_locked_zeros(*shapes["sdr"])[0]
        p = a.ctypes.data_as(C.POINTER(C.c_float))
        return lambda: g._check(g.L.ycge_render_frame(g.ctx, p, None))
    a = g._page_locked_zeros(*shapes["ansi"])[0]
    p = a.ctypes.data_as(U8P)
    return lambda: g._check(g.L.ycge_render_frame_chexels(g.ctx, None, None, p, None, None))


def part_rate(out: Path, rounds: int, frames: int):
    g = renderer(4)
    fns = {f: frame_fn(g, f) for f in FORMS}
    for f in FORMS:                      # warm-up: code objects, buffers, schedules
        for _ in range(5):
            fns[f]()
    per = {f: [] for f in FORMS}
    for r in range(rounds):
        order = list(FORMS) if r % 2 == 0 else list(reversed(FORMS))
        for f in order:
            t0 = time.perf_counter()
            for _ in range(frames):
                fns[f]()
            per[f].append((time.perf_counter() - t0) * 1e3 / frames)
    n = g.fbW * g.fbH
    res = {"config": 4, "framebuffer": [g.fbW, g.fbH], "console": [g.fbW + 1, g.fbH + 1], "rounds": rounds, "frames_per_round": frames,
           "stream_bytes": fns["ansi stream"](), "stream_bound": g.ansi_stream_bound(g.fbW + 1, g.fbH + 1, g.L),
           "bytes_read_back_other_forms": {"sdr": 24 * n, "chexels ansi": 2 * n},
           "ms_per_frame": {f: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for f, v in per.items()}}
    g.close()
    print(json.dumps(res), flush=True)
    (out / "rate.json").write_text(json.dumps(res, indent=1))


def part_bytes(out: Path, frames: int = 4):
    res = {}
    for n in (1, 2, 3, 4, 5):
        g = renderer(n)
        fn = frame_fn(g, "ansi stream")
        lens = [fn() for _ in range(frames)]
        res[f"config {n}"] = {"framebuffer": [g.fbW, g.fbH], "console": [g.fbW + 1, g.fbH + 1], "stream_bytes_per_frame": lens,
                              "bound": g.ansi_stream_bound(g.fbW + 1, g.fbH + 1, g.L)}
        g.close()
    print(json.dumps(res), flush=True)
    (out / "bytes.json").write_text(json.dumps(res, indent=1))


def part_kernel(out: Path):
    g = renderer(4)
    fn = frame_fn(g, "ansi stream")
    for _ in range(20):
        fn()
    g.close()


KERNELS = ("k_count", "k_scan", "k_write", "k_encode_chexels", "k_tonemap")      # (ycge_ansi_cells.hip.h's full-stream kernels, whichever colour form)


def kernel_rows(path):
    """per kernel: calls and µs, from the rocprofv3 --kernel-trace run's rocpd database (.db) or its kernel_stats.csv"""
    path = Path(path)
    if path.suffix == ".db":
        import sqlite3
        by = {}
        for n, d in sqlite3.connect(str(path)).execute("select name, duration from kernels"):
            k = next((k for k in KERNELS if k in n), None)
            if k:
                by.setdefault(k, []).append(d / 1e3)
        return [{"name": n, "calls": len(v), "median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                for n, v in sorted(by.items())]
    import csv
    return [{"name": r["Name"], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
             "max_us": float(r["MaxNs"]) / 1e3}
            for r in csv.DictReader(open(path)) if any(k in r.get("Name", "") for k in KERNELS)]


def part_merge(out: Path, kernel_stats, bench_logs=()):
    m = {"what": "the ANSI escape stream on the device (ycge_render_frame_ansi) on one MI355X; profiles/ansi_rate.py",
         "not_measured": "the host time of ANSITerminalRenderer.Render() in .NET, and the C# presenter (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    for part in ("rate", "bytes"):
        p = out / f"{part}.json"
        m[part] = json.loads(p.read_text()) if p.exists() else None
    if kernel_stats and Path(kernel_stats).exists():
        m["kernel_rocprofv3"] = kernel_rows(kernel_stats)
    if bench_logs:                  # bench.py on the parent and on this tree, alternating in the same job
        ab = {}
        for p in sorted(bench_logs):
            line = next((ln for ln in Path(p).read_text().splitlines() if '"value"' in ln), None)
            if line:
                d = json.loads(line[line.index("{"):])
                ab.setdefault("parent" if "parent" in Path(p).name else "branch", []).append({"Mrays_s": d["value"], "ms_per_step": d["ms_per_step"]})
        m["bench_ab"] = ab
    (ROOT / "profiles" / "ansi_rate.json").write_text(json.dumps(m, indent=1) + "\n")
    print(json.dumps(m)[:4000])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("rate", "bytes", "kernel", "merge"), required=True)
    ap.add_argument("--out", required=True, help="directory for the parts' JSON (outside the tree, or one git ignores)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--bench-logs", nargs="*", default=(), help="merge: bench_parent_*.log / bench_branch_*.log of the same job")
    a = ap.parse_args()
    out = Path(a.out); out.mkdir(parents=True, exist_ok=True)
    if a.part == "rate": part_rate(out, a.rounds, a.frames)
    elif a.part == "bytes": part_bytes(out)
    elif a.part == "kernel": part_kernel(out)
    else: part_merge(out, a.kernel_stats, a.bench_logs)
