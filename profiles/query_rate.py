"""Scene queries (ycge_scene_hit / ycge_scene_occluded): latency of small calls and throughput of large batches, one GPU.

    python profiles/query_rate.py --part latency    --out DIR     8-ray ycge_scene_hit calls, median / p99, configs 5 (dark) and 4, with no frame in
                                                                  flight and with a FrameLate-style frame in flight (ycge_render_frame_async_sdr)
    python profiles/query_rate.py --part throughput --out DIR     1 M-ray batches (random rays; a frame's primary rays) on configs 3, 4, 5, end to end
                                                                  (host arrays in, results out), and the oracle's rate on the same batch
    python profiles/query_rate.py --part merge      --out DIR [--kernel-stats FILE] [--suite-log LOG] [--bench-logs LOG ...]
                                                                  -> profiles/query_rate.json

Each part is its own process (the job script gives every one a time limit of its own); the kernel time comes from a separate
`rocprofv3 --kernel-trace --stats -- python profiles/query_rate.py --part throughput --quick` run, whose output (rocpd .db or kernel_stats.csv) the merge reads.
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

F32 = np.float32
FLT_MAX = F32(3.4028234663852886e38)


def renderer_for(cfg, t01=0.25, capture_debug=False):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(cfg, t01=t01)
    flat = flatten(sc)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss, capture_debug=capture_debug)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    g.SetFov(pose.get("fov", 45.0))
    return sc, flat, g, (w, h, ss, pose)


def scene_bounds(g):
    from yetanotherconsolegameengine_amd import abi
    nodes = g.accel(abi.ACCEL_SCENE_NODES)
    lo = np.clip(nodes["min"].min(axis=0), -200, 200).astype(F32)
    hi = np.clip(nodes["max"].max(axis=0), -200, 200).astype(F32)
    return lo, np.maximum(hi, lo + F32(1.0))


def random_batch(g, n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(g)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(F32)
    d = rng.normal(size=(n, 3)).astype(F32)
    return o, d


def stats_ms(t):
    t = np.asarray(t) * 1e3
    return {"median_ms": float(np.median(t)), "p99_ms": float(np.percentile(t, 99)), "min_ms": float(t.min()), "calls": int(t.size)}


def part_latency(out: Path):
    res = {}
    for cfg, t01, name in ((5, 0.25, "config5_dark"), (4, 0.25, "config4")):
        sc, flat, g, (w, h, ss, pose) = renderer_for(cfg, t01)
        o, d = random_batch(g, 8, 1)
        for _ in range(20):
            g.Hit(o, d)
        g.TryFlipAndBlit()
        t_idle = []
        for _ in range(400):
            t0 = time.perf_counter(); g.Hit(o, d); t_idle.append(time.perf_counter() - t0)
        # FrameLate: the frame of this call is queued (post stage and read-back included), the host's Update asks its probes, the next call waits
        for k in range(4):
            g.RenderAsync(sdr_slot=k % 2); g.Hit(o, d); g.Wait()
        t_fl, outstanding, t_frame = [], [], []
        for k in range(200):
            t0 = time.perf_counter()
            g.RenderAsync(sdr_slot=k % 2)
            t1 = time.perf_counter(); g.Hit(o, d); t2 = time.perf_counter()
            outstanding.append(g.flight_info()["frames_outstanding"])
            g.Wait()
            t_fl.append(t2 - t1); t_frame.append(time.perf_counter() - t0)
        # the same frames without the probe: what the frame costs the caller's loop on its own
        t_frame0 = []
        for k in range(200):
            t0 = time.perf_counter(); g.RenderAsync(sdr_slot=k % 2); g.Wait(); t_frame0.append(time.perf_counter() - t0)
        res[name] = {"rays_per_call": 8, "no_frame_in_flight": stats_ms(t_idle), "frame_in_flight": stats_ms(t_fl),
                     "frames_outstanding_after_query": int(min(outstanding)),
                     "loop_ms_with_query": stats_ms(t_frame), "loop_ms_without_query": stats_ms(t_frame0)}
        print(name, json.dumps(res[name]), flush=True)
        g.close()
    (out / "latency.json").write_text(json.dumps(res, indent=1))


def part_throughput(out: Path, quick: bool):
    from yetanotherconsolegameengine_amd import abi
    import oracle_binding as ob
    res = {}
    n = 1 << 20
    for cfg in (3, 4, 5):
        sc, flat, g, (w, h, ss, pose) = renderer_for(cfg, 0.5, capture_debug=True)
        g.TryFlipAndBlit()
        r6 = g.read(abi.BUF_RAYS).reshape(-1, 6)
        reps = int(np.ceil(n / r6.shape[0]))
        prim = np.tile(r6, (reps, 1))[:n]
        o, d = random_batch(g, n, cfg)
        entry = {}
        for kind, (oo, dd) in (("random", (o, d)), ("primary", (prim[:, 0:3], prim[:, 3:6]))):
            oo = np.ascontiguousarray(oo); dd = np.ascontiguousarray(dd)
            g.Hit(oo, dd)                               # (buffers grown, code loaded)
            g.Occluded(oo, dd)
            tt, to = [], []
            for _ in range(2 if quick else 5):
                t0 = time.perf_counter(); hits, ids = g.Hit(oo, dd); tt.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); occ = g.Occluded(oo, dd); to.append(time.perf_counter() - t0)
            e = {"rays": n, "hit_fraction": float((ids[:, 0] >= 0).mean()),
                 "hit_mrays_s_end_to_end": n / min(tt) / 1e6, "occluded_mrays_s_end_to_end": n / min(to) / 1e6,
                 "hit_ms": min(tt) * 1e3, "occluded_ms": min(to) * 1e3}
            if not quick:
                # the oracle (one CPU thread, the reference's scalar walk) on the first 65 536 rays of the same batch
                L = ob.lib()
                L.orc_scene_hit_many.restype = C.c_int
                L.orc_scene_hit_many.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p]
                orc = ob.OracleRenderer(sc, w, h, ss, pose, flat=flat)
                m = 1 << 16
                od = np.ascontiguousarray(np.concatenate([oo[:m], dd[:m]], axis=1))
                tq = np.zeros(m, F32); pq = np.zeros(m, np.int32)
                t0 = time.perf_counter()
                L.orc_scene_hit_many(orc.ctx, od.ctypes.data_as(C.POINTER(C.c_float)), m, 0.001, float(FLT_MAX), tq.ctypes.data_as(C.POINTER(C.c_float)), pq.ctypes.data_as(C.POINTER(C.c_int32)), None)
                dt = time.perf_counter() - t0
                orc.close()
                e["oracle_mrays_s_one_thread"] = m / dt / 1e6
                e["oracle_equal_objects_first_64k"] = bool(np.array_equal(pq, ids[:m, 0]))
            entry[kind] = e
        res[f"config{cfg}"] = entry
        print(cfg, json.dumps(entry), flush=True)
        g.close()
    (out / ("throughput_quick.json" if quick else "throughput.json")).write_text(json.dumps(res, indent=1))


def kernel_rows(path):
    """k_query dispatches of the rocprofv3 --kernel-trace run, in order: from its rocpd database (.db) or its kernel_stats.csv"""
    path = Path(path)
    if path.suffix == ".db":
        import sqlite3
        db = sqlite3.connect(str(path))
        return [{"name": n.split("(")[0], "grid": int(gx), "ns": int(d)}
                for n, gx, d in db.execute("select name, grid_x, duration from kernels where name like '%k_query%' order by start")]
    import csv
    return [{"name": r["Name"], "calls": int(r["Calls"]), "avg_ns": float(r["AverageNs"]), "min_ns": float(r["MinNs"])}
            for r in csv.DictReader(open(path)) if "k_query" in r.get("Name", "")]


def part_merge(out: Path, kernel_stats, suite_log=None, bench_logs=()):
    m = {"what": "scene queries (ycge_scene_hit / ycge_scene_occluded) on one MI355X; profiles/query_rate.py"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    for name in ("latency", "throughput"):
        p = out / f"{name}.json"
        m[name] = json.loads(p.read_text()) if p.exists() else None
    if kernel_stats and Path(kernel_stats).exists():
        rows = kernel_rows(kernel_stats)
        if rows and "ns" in rows[0]:
            # the --quick throughput run: per config (3, 4, 5) and batch (random, primary) one warm-up pair and two timed pairs of
            # (ycge_scene_hit, ycge_scene_occluded) launches on 1 M rays; the fastest of the three per launch kind
            labels = [(c, k, q) for c in (3, 4, 5) for k in ("random", "primary") for _ in range(3) for q in ("hit", "occluded")]
            ks = {}
            if len(rows) == len(labels):
                for (c, k, q), r in zip(labels, rows):
                    e = ks.setdefault(f"config{c}", {}).setdefault(k, {})
                    e[q + "_kernel_ms"] = min(e.get(q + "_kernel_ms", 1e9), r["ns"] / 1e6)
                for c in ks.values():
                    for e in c.values():
                        e["hit_kernel_grays_s"] = (1 << 20) / (e["hit_kernel_ms"] * 1e-3) / 1e9
                        e["occluded_kernel_grays_s"] = (1 << 20) / (e["occluded_kernel_ms"] * 1e-3) / 1e9
            m["kernel_rocprofv3"] = {"resident_lanes": rows[0]["grid"], "by_batch": ks, "dispatches": rows}
        else:
            m["kernel_rocprofv3"] = rows
    if suite_log and Path(suite_log).exists():          # the GPU suite's summary line from the same job
        m["gpu_suite"] = [ln.strip() for ln in Path(suite_log).read_text().splitlines() if " passed" in ln][-1:]
    if bench_logs:                                        # headline A/B in the same job: bench.py on the parent and on this tree, alternating
        ab = {}
        for p in sorted(bench_logs):
            txt = Path(p).read_text()
            line = next((ln for ln in txt.splitlines() if '"value"' in ln), None)
            if line:
                d = json.loads(line[line.index("{"):])
                ab.setdefault("parent" if "parent" in Path(p).name else "branch", []).append({"Mrays_s": d["value"], "ms_per_step": d["ms_per_step"]})
        m["bench_ab"] = ab
    (ROOT / "profiles" / "query_rate.json").write_text(json.dumps(m, indent=1) + "\n")
    print(json.dumps(m)[:4000])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("latency", "throughput", "merge"), required=True)
    ap.add_argument("--out", required=True, help="directory for the parts' JSON (outside the tree, or one git ignores)")
    ap.add_argument("--quick", action="store_true", help="throughput: two repetitions, no oracle (the rocprofv3 run)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--suite-log", default=None, help="merge: the GPU suite's pytest log of the same job")
    ap.add_argument("--bench-logs", nargs="*", default=(), help="merge: bench_parent_*.log / bench_branch_*.log of the same job")
    a = ap.parse_args()
    out = Path(a.out); out.mkdir(parents=True, exist_ok=True)
    if a.part == "latency": part_latency(out)
    elif a.part == "throughput": part_throughput(out, a.quick)
    else: part_merge(out, a.kernel_stats, a.suite_log, a.bench_logs)
