"""Device chexel colours (ycge_render_frame_chexels): what a frame costs when the host asks for presenter bytes instead of, or beside,
the f32 SDR array.  Config 4 (1920 x 540 console), one GPU, one process, the forms alternated round by round.

    python profiles/chexel_rate.py --part rate   --out DIR [--rounds R --frames K --parent-lib PATH]   ms/frame of each form -> DIR/rate.json
    python profiles/chexel_rate.py --part kernel --out DIR                           a short run of the all-outputs form (for rocprofv3)
    python profiles/chexel_rate.py --part merge  --out DIR [--kernel-stats FILE] [--bench-logs LOG ...]   -> profiles/chexel_rate.json

Forms: `sdr` is ycge_render_frame(sdr) - today's frame; the others are ycge_render_frame_chexels with the outputs named.  Every
destination is page-locked memory of the library (as the C# wrapper's), so the read-back is a plain DMA.  A frame's time is the host
clock around the call, which returns with the frame in the caller's arrays.  The kernel time of k_encode_chexels comes from a separate
`rocprofv3 --kernel-trace --stats -- python profiles/chexel_rate.py --part kernel` run, whose rocpd database (or kernel_stats.csv) the merge reads.
With --parent-lib, the parent commit's library (built elsewhere from the parent's sources) is loaded beside the product's: two legs of
the parent and one of the product run every form, alternated round by round, and rate.json gets `against_parent` (parent_check below).
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

FORMS = {"sdr": ("sdr",), "color16": ("color16",), "rgba": ("rgba",), "sdr+color16": ("sdr", "color16"),
         "all four": ("sdr", "color16", "ansi", "rgba")}


def renderer(lib=None):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(4)
    g = RaytraceRenderer(flatten(sc), w, h, pose.get("fov", 45.0), ss, lib=lib)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    return g


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


def frame_fn(g, form):
    """a callable that renders one frame of `form` into page-locked arrays of the library"""
    arrays = {k: g._page_locked_zeros(shp, dt)[0] for k, (shp, dt) in g.chexel_shapes().items() if k in FORMS[form]}
    if form == "sdr":
        p = arrays["sdr"].ctypes.data_as(C.POINTER(C.c_float))
        return lambda: g._check(g.L.ycge_render_frame(g.ctx, p, None)), arrays
    ptrs = g._chexel_pointers(arrays)
    return lambda: g._check(g.L.ycge_render_frame_chexels(g.ctx, *ptrs, None)), arrays


def against_parent(parent_lib, rounds: int, frames: int):
    from yetanotherconsolegameengine_amd import abi
    P = abi.load_library(parent_lib)
    libs = {"parent A": P, "branch": None, "parent B": P}
    per = {(b, f): [] for b in libs for f in FORMS}
    for r in range(rounds):
        for b in (list(libs) if r % 2 == 0 else list(libs)[::-1]):
            g = renderer(libs[b])
            fns = {f: frame_fn(g, f)[0] for f in FORMS}
            for f in FORMS:
                for _ in range(5):
                    fns[f]()
            for f in FORMS:
                t0 = time.perf_counter()
                for _ in range(frames):
                    fns[f]()
                per[(b, f)].append((time.perf_counter() - t0) * 1e3 / frames)
            g.close()
    return parent_check(per)


def part_rate(out: Path, rounds: int, frames: int, parent_lib=None):
    g = renderer()
    fns = {f: frame_fn(g, f)[0] for f in FORMS}
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
    res = {"config": 4, "console": [g.fbW, g.fbH], "rounds": rounds, "frames_per_round": frames,
           "bytes_read_back": {f: sum({"sdr": 24, "color16": 1, "ansi": 2, "rgba": 8}[k] * n for k in FORMS[f]) for f in FORMS},
           "ms_per_frame": {f: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for f, v in per.items()}}
    g.close()
    if parent_lib:
        res["against_parent"] = against_parent(parent_lib, rounds, frames)
    print(json.dumps(res), flush=True)
    (out / "rate.json").write_text(json.dumps(res, indent=1))


def part_kernel(out: Path):
    g = renderer()
    fn, _ = frame_fn(g, "all four")
    for _ in range(20):
        fn()
    c16, _ = frame_fn(g, "color16")
    for _ in range(20):
        c16()
    g.close()


KERNELS = ("k_encode_chexels", "k_tonemap")


def kernel_rows(path):
    """per kernel (k_encode_chexels by instantiation, the tonemap beside it): calls and µs, from the rocprofv3 --kernel-trace run's rocpd
    database (.db) or its kernel_stats.csv"""
    path = Path(path)
    if path.suffix == ".db":
        import sqlite3
        by = {}
        for n, d in sqlite3.connect(str(path)).execute("select name, duration from kernels"):
            if any(k in n for k in KERNELS):
                form = "<true>" if ("<true>" in n or "ILb1E" in n) else "<false>" if ("<false>" in n or "ILb0E" in n) else ""
                by.setdefault(next(k for k in KERNELS if k in n) + form, []).append(d / 1e3)
        return [{"name": n, "calls": len(v), "median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
                for n, v in sorted(by.items())]
    import csv
    return [{"name": r["Name"], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
             "max_us": float(r["MaxNs"]) / 1e3}
            for r in csv.DictReader(open(path)) if any(k in r.get("Name", "") for k in KERNELS)]


def part_merge(out: Path, kernel_stats, bench_logs=()):
    m = {"what": "device chexel colours (ycge_render_frame_chexels) on one MI355X, config 4 at 1920 x 540; profiles/chexel_rate.py"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    p = out / "rate.json"
    m["rate"] = json.loads(p.read_text()) if p.exists() else None
    if kernel_stats and Path(kernel_stats).exists():
        m["kernel_rocprofv3"] = kernel_rows(kernel_stats)
    if bench_logs:                  # the headline A/B of the same job: bench.py on the parent and on this tree, alternating
        ab = {}
        for p in sorted(bench_logs):
            line = next((ln for ln in Path(p).read_text().splitlines() if '"value"' in ln), None)
            if line:
                d = json.loads(line[line.index("{"):])
                ab.setdefault("parent" if "parent" in Path(p).name else "branch", []).append({"Mrays_s": d["value"], "ms_per_step": d["ms_per_step"]})
        m["bench_ab"] = ab
    (ROOT / "profiles" / "chexel_rate.json").write_text(json.dumps(m, indent=1) + "\n")
    print(json.dumps(m)[:4000])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("rate", "kernel", "merge"), required=True)
    ap.add_argument("--out", required=True, help="directory for the parts' JSON (outside the tree, or one git ignores)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--parent-lib", default=None, help="rate: the parent commit's library, measured beside the product's")
    ap.add_argument("--bench-logs", nargs="*", default=(), help="merge: bench_parent_*.log / bench_branch_*.log of the same job")
    a = ap.parse_args()
    out = Path(a.out); out.mkdir(parents=True, exist_ok=True)
    if a.part == "rate": part_rate(out, a.rounds, a.frames, a.parent_lib)
    elif a.part == "kernel": part_kernel(out)
    else: part_merge(out, a.kernel_stats, a.bench_logs)
