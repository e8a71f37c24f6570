"""Many bodies a tick (ycge_volume_bodies_tick) on the config-5 voxel world, one GPU: what a call costs by route and batch size, and what
it does to a frame and to the single tick.

    python profiles/volume_bodies_rate.py --out DIR [--parent-lib PATH] [--rounds R] [--frames F]     -> DIR/volume_bodies_rate.json

The bodies: a square grid of positions around the config's pose, 1.5 apart (some 108 x 108 units of the island), auto-placed by their
first tick and ticked until they rest or 60 ticks have passed; the 4096 centre-most that came to rest are kept, a batch of n is the n
centre-most of them.  Every repetition starts from copies of those bodies, so it does the same work.  n = 1, 16, 64, 256, 1024, 4096, with
2 and 4 for the crossover and 2048 and 3072 around what can be resident.  Two tick shapes: a quiet tick (no moves) and a tick with one walking move a body (6 units/s for 16 ms, heading -z).  Three
routes, alternated round by round in one process:

    device    ycge_volume_bodies_tick                        one staged copy up, one launch of n workgroups, one copy back, one synchronise
    host      the same call with YCGE_CAMERA_HOST=1          the stepper on the host, a round of all bodies' windows one batch of scene queries
    singles   n calls of ycge_volume_camera_tick             the only way before this export (default shape)

Each cell: median, min and p99 of the wall time of a call (singles: of the n calls together) in microseconds, and bodies a second from
the median.  Then the n from which the batch beats the singles, and the per-body time by n.
Then the period of a synchronous config-5 frame (1920 x 540, ss 2) with a 256-body quiet tick after every frame and without, and - with
--parent-lib, a library built from the parent commit - the same frames and the single tick through that library in the same run.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

SIZES = (1, 2, 4, 16, 64, 256, 1024, 2048, 3072, 4096)          # the issue's six, 2 and 4 for the crossover, 2048 and 3072 around what can be resident


def stats_us(t):
    t = np.asarray(t) * 1e6
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "p99_us": float(np.percentile(t, 99)), "calls": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    from yetanotherconsolegameengine_amd import abi, build, scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten

    L = abi.load_library()
    sc, w, h, ss, pose = scenes.config_scene(5, t01=0.5)
    flat = flatten(sc)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    world = abi.CameraWorld(256.0, 64.0, 1.0)
    walk = abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, 0.0, -6.0 * 0.016)

    # the settled bodies: a grid of candidates, ticked until they rest or 60 ticks have passed; the max(SIZES) centre-most that came to rest
    # are kept (a body that never rests - over water, below the world - runs a chain many times a resting one's, and a launch lasts as long
    # as its slowest body), every smaller n its centre-most bodies
    side = int(np.ceil(np.sqrt(max(SIZES) * 1.25)))
    px, py, pz = pose["pos"]
    cells = sorted(((i - side / 2) ** 2 + (j - side / 2) ** 2, i, j) for i in range(side) for j in range(side))
    rested = []
    for at in range(0, len(cells), max(SIZES)):
        part = cells[at:at + max(SIZES)]
        cand = (abi.CameraBody * len(part))()
        for k, (_, i, j) in enumerate(part):
            cand[k].pos[:] = [px + 1.5 * (i - side / 2), py, pz + 1.5 * (j - side / 2)]
        none = [[] for _ in part]
        for t in range(60):
            results, _ = g.BodiesTick(cand, world, none, 16.0)
            assert all(s == 0 for s, _ in results)
            if all(b.is_grounded for b in cand): break
        rested += [bytes(b) for b in cand if b.is_grounded]
    candidates, grounded = len(cells), len(rested)
    assert grounded >= max(SIZES), (grounded, candidates)
    settled = (abi.CameraBody * max(SIZES)).from_buffer_copy(b"".join(rested[:max(SIZES)]))

    def fresh(n):
        b = (abi.CameraBody * n)()
        C.memmove(b, settled, C.sizeof(b))
        return b

    def call(route, lib, ctx, n, moves):
        """one repetition: (seconds, bytes of the bodies afterwards)"""
        b = fresh(n)
        if route == "singles":
            info = abi.CameraTickInfo()
            recs = (abi.CameraMove * 1)(*moves) if moves else None
            t0 = time.perf_counter()
            for i in range(n):
                rc = lib.ycge_volume_camera_tick(ctx, C.byref(b[i]), C.byref(world), recs, len(moves), 16.0, 1, C.byref(info))
                assert rc == 0, rc
            return time.perf_counter() - t0, bytes(b)
        recs = (abi.CameraMove * max(1, n * len(moves)))(*(list(moves) * n))
        first = (C.c_int32 * (n + 1))(*[i * len(moves) for i in range(n + 1)])
        results = (abi.BodyResult * n)()
        info = (abi.CameraTickInfo * n)()
        if route == "host": os.environ["YCGE_CAMERA_HOST"] = "1"
        else: os.environ.pop("YCGE_CAMERA_HOST", None)
        t0 = time.perf_counter()
        rc = lib.ycge_volume_bodies_tick(ctx, b, None, n, C.byref(world), recs if moves else None, first, 16.0, 1, results, info)
        dt = time.perf_counter() - t0
        os.environ.pop("YCGE_CAMERA_HOST", None)
        assert rc == 0 and all(r.status == 0 for r in results), (route, rc, L.ycge_last_error(ctx))
        if route == "device":                             # the chain of the slowest body bounds a launch from below
            chains[(n, len(moves))] = {"max_windows": max(int(i.windows) for i in info), "max_rays_walked": max(int(i.rays_walked) for i in info),
                                       "rays_walked": sum(int(i.rays_walked) for i in info)}
        return dt, bytes(b)

    chains = {}
    routes = ("device", "host", "singles")
    shapes = {"quiet": [], "walk": [walk]}
    times = {(r, s, n): [] for r in routes for s in shapes for n in SIZES}
    for rnd in range(a.rounds + 1):                      # round 0 warms every route, shape and size up and is dropped
        for n in SIZES:
            reps = {"device": max(3, min(60, 4000 // n)), "host": max(2, min(30, 600 // n)), "singles": max(2, min(30, 600 // n))}
            for route in routes:
                for s, moves in shapes.items():
                    ends = set()
                    for _ in range(reps[route] if rnd else 2):
                        dt, end = call(route, L, g.ctx, n, moves)
                        if rnd: times[(route, s, n)].append(dt)
                        ends.add(end)
                    assert len(ends) == 1, (route, s, n)
            for s, moves in shapes.items():              # the three routes leave the same bodies
                assert call("device", L, g.ctx, n, moves)[1] == call("host", L, g.ctx, n, moves)[1] == call("singles", L, g.ctx, n, moves)[1], (s, n)
    res = {"bodies_settled": {"candidates": candidates, "came_to_rest": grounded, "kept": max(SIZES)}, "calls": {}}
    for r in routes:
        res["calls"][r] = {s: {str(n): dict(stats_us(times[(r, s, n)]), bodies_per_second=n / float(np.median(times[(r, s, n)]))) for n in SIZES} for s in shapes}
    med = lambda r, s, n: float(np.median(times[(r, s, n)]))
    res["batch_beats_singles_from_n"] = {s: next((n for n in SIZES if med("device", s, n) < med("singles", s, n)), None) for s in shapes}
    res["device_chains"] = {s: {str(n): chains[(n, len(moves))] for n in SIZES} for s, moves in shapes.items()}
    res["device_us_per_body"] = {s: {str(n): med("device", s, n) * 1e6 / n for n in SIZES} for s in shapes}
    # 3 waves a SIMD by the compiler's figures (profiles/volume_bodies_resources.txt), 4 SIMDs a CU: the workgroups that can be resident
    res["resident_workgroups_per_cu_by_compiler_figures"] = 3 * 4

    # the frame's period with a 256-body quiet tick after every frame and without; the single tick; the parent commit's library beside both
    libs = {"this": (L, g)}
    if a.parent_lib:
        Lp = abi.bind(C.CDLL(str(a.parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n != "ycge_volume_bodies_tick"])    # (the parent has no such export)
        gp = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss, lib=Lp)
        gp.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        libs["parent"] = (Lp, gp)
    cases = [("this", False), ("this", True)] + ([("parent", False)] if a.parent_lib else [])
    periods = {c: [] for c in cases}
    for rnd in range(a.rounds + 1):
        for c in cases:
            lib, gg = libs[c[0]]
            for _ in range(a.frames if rnd else 5):
                t0 = time.perf_counter()
                gg.TryFlipAndBlit()
                if c[1]: call("device", lib, gg.ctx, 256, [])
                dt = time.perf_counter() - t0
                if rnd: periods[c].append(dt)
    res["frame_period"] = {f"{lib}{'+256 bodies' if t else ''}": stats_us(v) for (lib, t), v in periods.items()}
    single = {(lib, s): [] for lib in libs for s in shapes}
    for rnd in range(a.rounds + 1):
        for lib, (ll, gg) in libs.items():
            for s, moves in shapes.items():
                for _ in range(200 if rnd else 10):
                    dt, _ = call("singles", ll, gg.ctx, 1, moves)
                    if rnd: single[(lib, s)].append(dt)
    res["single_tick"] = {lib: {s: stats_us(single[(lib, s)]) for s in shapes} for lib in libs}
    res["source_hash"] = build.source_hash()
    res["device"] = str(g.device_info())
    (out / "volume_bodies_rate.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
