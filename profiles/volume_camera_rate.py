"""The camera tick (ycge_volume_camera_tick) on the config-5 voxel world, one GPU: what a tick costs by route, and what it does to a frame.

    python profiles/volume_camera_rate.py --out DIR [--parent-lib PATH] [--rounds R] [--ticks N] [--frames F]     -> DIR/volume_camera_rate.json

Three tick shapes from the same body each time (a tick is a function of its body, so every repetition does the same work): a quiet tick
(no moves), a tick with one walking move (6 units/s for 16 ms, along a heading that meets nothing), a tick with such a move towards a wall (the body is first flown
along a heading until a micro-step is blocked and the push-out has set it 0.66 off the wall; absent when none of eight headings meets a
wall).  Three routes, alternated round by
round in one process:

    device   ycge_volume_camera_tick                       one launch, one read-back, one synchronise
    host     the same call with YCGE_CAMERA_HOST=1         the stepper on the host, a window a batch of scene queries
    per_ray  ycge_test_camera_tick_host, serial order      what a host has today: one ycge_scene_hit call per ray, here through a ctypes callback
                                                           (a few microseconds of Python per ray are inside the figure)

Each cell: median, min and p99 of the wall time of a call in microseconds, with rays_committed, rays_walked, windows and what the tick
met (micro-steps, blocked micro-steps, push-outs) beside it.
Then the period of a synchronous config-5 frame (1920 x 540, ss 2) with and without a quiet tick between frames, and - with
--parent-lib, a library built from the parent commit - the same frames through that library in the same run, rounds alternated.
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


def stats_us(t):
    t = np.asarray(t) * 1e6
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "p99_us": float(np.percentile(t, 99)), "calls": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    from yetanotherconsolegameengine_amd import abi, build, scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten

    L = abi.load_library()
    for name, (res, args) in abi.CAMERA_HOOK_PROTOTYPES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    sc, w, h, ss, pose = scenes.config_scene(5, t01=0.5)
    flat = flatten(sc)
    g = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    world = abi.CameraWorld(256.0, 64.0, 1.0)

    def body_at(pos):
        b = abi.CameraBody()
        b.pos[:] = [float(v) for v in pos]
        b.auto_placed = 1
        return b

    def copy(b):
        c = abi.CameraBody()
        C.memmove(C.byref(c), C.byref(b), C.sizeof(b))
        return c

    # the resting body: dropped from the pose until it is grounded
    rest = body_at(pose["pos"])
    for _ in range(200):
        g.CameraTick(rest, world, [], 16.0)
        if rest.is_grounded: break
    # the walking move: the first of eight headings along which one step from rest meets nothing (no blocked micro-step, no push-out)
    walk = abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, 0.0, -6.0 * 0.016)
    for k in range(8):
        ang = 2 * np.pi * k / 8
        m = abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, float(np.sin(ang)) * 6.0 * 0.016, float(-np.cos(ang)) * 6.0 * 0.016)
        info = g.CameraTick(copy(rest), world, [m], 16.0)
        if not info["blocked_steps"] and not info["push_outs"]:
            walk = m
            break
    # a wall: fly along one of eight headings until a micro-step is blocked
    at_wall, wall_move = None, None
    for k in range(8):
        ang = 2 * np.pi * k / 8
        dx, dz = float(np.sin(ang)), float(-np.cos(ang))
        b = copy(rest)
        for _ in range(40):
            info = g.CameraTick(b, world, [abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, dx * 2.0, dz * 2.0)], 16.0)
            if info["blocked_steps"]:
                break
        if info["blocked_steps"]:
            at_wall, wall_move = b, abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, dx * 6.0 * 0.016, dz * 6.0 * 0.016)
            break
    shapes = {"quiet": (rest, []), "walk": (rest, [walk])}
    if at_wall is not None:
        shapes["wall"] = (at_wall, [wall_move])

    hits, ids = (C.c_float * 10)(), (C.c_int32 * 2)()

    def per_ray(_user, ray, rec):
        if L.ycge_scene_hit(g.ctx, ray, 1, hits, ids) != 0: raise RuntimeError("ycge_scene_hit")
        if ids[0] < 0: return 0
        for i in range(7): rec[i] = hits[i]
        return 1
    cb = abi.CAMERA_HIT_FN(per_ray)

    def tick(route, b, moves):
        recs = (abi.CameraMove * max(1, len(moves)))(*moves)
        info = abi.CameraTickInfo()
        if route == "per_ray":
            t0 = time.perf_counter()
            rc = L.ycge_test_camera_tick_host(C.byref(b), C.byref(world), recs, len(moves), 16.0, 1, C.byref(info), cb, None, 0, None, 0)
            dt = time.perf_counter() - t0
        else:
            if route == "host": os.environ["YCGE_CAMERA_HOST"] = "1"
            else: os.environ.pop("YCGE_CAMERA_HOST", None)
            t0 = time.perf_counter()
            rc = L.ycge_volume_camera_tick(g.ctx, C.byref(b), C.byref(world), recs, len(moves), 16.0, 1, C.byref(info))
            dt = time.perf_counter() - t0
            os.environ.pop("YCGE_CAMERA_HOST", None)
        assert rc == 0, (route, rc, L.ycge_last_error(g.ctx))
        return dt, info

    routes = ("device", "host", "per_ray")
    times = {r: {s: [] for s in shapes} for r in routes}
    work, bodies = {}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms every route and shape up and is dropped
        for route in routes:
            n = a.ticks if route != "per_ray" else max(10, a.ticks // 10)
            for s, (b0, moves) in shapes.items():
                for _ in range(n if rnd else 5):
                    b = copy(b0)
                    dt, info = tick(route, b, moves)
                    if rnd: times[route][s].append(dt)
                work[(route, s)] = {k: int(getattr(info, k)) for k in ("rays_committed", "rays_walked", "windows", "micro_steps", "blocked_steps", "push_outs")}
                bodies[(route, s)] = bytes(b)
    for s in shapes:                                     # the three routes leave the same body
        assert bodies[("device", s)] == bodies[("host", s)] == bodies[("per_ray", s)], s
    res = {"ticks": {r: {s: dict(stats_us(times[r][s]), **work[(r, s)]) for s in shapes} for r in routes}, "wall_found": at_wall is not None}

    # the frame's period with and without a quiet tick between frames; the parent commit's library beside it
    libs = {"this": (L, g)}
    if a.parent_lib:
        Lp = abi.bind(C.CDLL(str(a.parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n != "ycge_volume_camera_tick"])    # (the parent has no such export)
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
                if c[1]:
                    b = copy(rest)
                    gg.CameraTick(b, world, [], 16.0)
                dt = time.perf_counter() - t0
                if rnd: periods[c].append(dt)
    res["frame_period"] = {f"{lib}{'+tick' if t else ''}": stats_us(v) for (lib, t), v in periods.items()}
    res["source_hash"] = build.source_hash()
    res["device"] = str(g.device_info())
    (out / "volume_camera_rate.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
