"""Chunk streaming (ycge_scene_attach_grids / ycge_scene_update_objects / ycge_scene_detach_grids) against the only other way to do
the same thing, ycge_scene_upload of the same final scene: config 5, the full world resident, one border crossing in x per tick.

    python profiles/stream_rate.py [--ticks N] [--small]     -> profiles/stream_rate.json

One process, one MI355X.  Per tick the camera column moves one chunk along x (back and forth): the far row of 17 x 8 chunk positions
leaves, a new row enters (air chunks skipped).  The streamed context makes the three calls, then a second context uploads the
equivalent flattened scene - the two legs alternate inside the run.  Only the library calls are timed (the Python flattening of
either leg is outside the clock); the split of the attach comes from ycge_debug_grid_pool_stats (host clock around each step,
every step ends in a stream synchronise), the tree build from ycge_debug_scene_bvh_stats.  Then the same tick between frames in flight.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np


def stats(t, scale=1e3):
    t = np.asarray(t, dtype=np.float64) * scale
    return {"median": float(np.median(t)), "p99": float(np.percentile(t, 99)), "min": float(t.min()), "n": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="the 96 x 128 x 96 world, view distance 1 (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stream_rate.json"))
    ap.add_argument("--merge-bench", nargs="*", default=None, help="bench_parent_*.log / bench_branch_*.log of the same job (bench.py, plain run, "
                    "alternating): added to the JSON at --out as bench_ab; nothing else runs")
    a = ap.parse_args()
    if a.merge_bench is not None:
        res = json.loads(Path(a.out).read_text())
        ab = {}
        for p in sorted(a.merge_bench):
            line = next((ln for ln in Path(p).read_text().splitlines() if '"value"' in ln), None)
            if line:
                d = json.loads(line[line.index("{"):])
                ab.setdefault("parent" if "parent" in Path(p).name else "branch", []).append({"Mrays_s": d["value"], "ms_per_step": d["ms_per_step"]})
        res["bench_ab"] = ab
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(ab))
        return
    from yetanotherconsolegameengine_amd import build, scenes, world_file
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import AmbientLight, Scene, VolumeGrid, flatten, vec3

    nx, ny, nz, view = (96, 128, 96, 1) if a.small else (544, 256, 544, 8)
    chunk = 32
    world = scenes.make_voxel_world(nx, ny, nz)
    wmin, voxel = (-nx // 2, 0.0, -nz // 2), (1.0, 1.0, 1.0)
    scene = Scene()
    scene.IsVolumeScene = True
    scene.Ambient = AmbientLight(vec3(1, 1, 1), 0.0)
    lights, top, bottom = scenes.sun_moon_lights(0.5)
    scene.Lights.extend(lights)
    scene.BackgroundTop, scene.BackgroundBottom = top, bottom
    loaded = {}
    col = world[nx // 2, :, nz // 2, 0]
    eye_y = float(int(np.nonzero(col)[0].max()) + 1) + 1.8

    def tick(x):
        return world_file.stream_view(scene, world, (x, eye_y, 0.0), wmin, voxel, chunk, view, scenes.VoxelMaterialLookup, loaded)

    tick(0.0)
    w, h, ss = (160, 90, 1) if a.small else (1920, 540, 2)
    g = RaytraceRenderer(flatten(scene), w, h, 45.0, ss)
    t = RaytraceRenderer(flatten(scene), w, h, 45.0, ss)
    for r in (g, t):
        r.SetCamera((0.0, eye_y, 0.0), 0.0, -0.2)
        r.TryFlipAndBlit()
    res = {"what": "chunk streaming against ycge_scene_upload on one MI355X; profiles/stream_rate.py", "build": build.source_hash(),
           "world": [nx, ny, nz], "view_distance_chunks": view, "resident_grids": len(loaded), "frame": [w, h, ss]}
    legs = {k: [] for k in ("tick_ms", "attach_ms", "update_ms", "detach_ms", "upload_ms", "stage_us", "h2d_us", "kernel_us", "readback_us", "tree_us",
                            "voxels", "chunks_in", "chunks_out", "raw_mb")}
    for k in range(a.warmup + a.ticks):
        x = 32.0 if k % 2 == 0 else 0.0
        added, removed = tick(x)
        g.StreamObjects(scene)
        eq = flatten(scene)
        t0 = time.perf_counter()
        rc = t.L.ycge_scene_upload(t.ctx, eq.byref())
        up = time.perf_counter() - t0
        t._check(rc); t.flat = eq
        if k < a.warmup:
            continue
        c, st, bv = g.stream_call_s, g.grid_pool_stats(), g.scene_bvh_stats()
        vox = int(sum(int(np.prod(loaded[key].Cells.shape[:3])) for key in added))
        for name, v in (("tick_ms", c["attach"] + c["update"] + c["detach"]), ("attach_ms", c["attach"]), ("update_ms", c["update"]), ("detach_ms", c["detach"]),
                        ("upload_ms", up)):
            legs[name].append(v)
        for name, v in (("stage_us", st["last_stage_us"]), ("h2d_us", st["last_h2d_us"]), ("kernel_us", st["last_kernel_us"]), ("readback_us", st["last_readback_us"]),
                        ("tree_us", bv["last_build_us"]), ("voxels", vox), ("chunks_in", len(added)), ("chunks_out", len(removed)), ("raw_mb", vox * 8 / 1e6)):
            legs[name].append(v)
    res["border_crossing"] = {k: stats(v) for k, v in legs.items() if k.endswith("_ms")}
    res["border_crossing"].update({k: stats(v, 1.0) for k, v in legs.items() if not k.endswith("_ms")})
    # the ticks that attached something (at the world's edge a crossing only detaches: the row that would enter lies outside the world)
    att = [i for i, v in enumerate(legs["voxels"]) if v > 0]
    res["attaching_ticks"] = {k: stats([legs[k][i] for i in att], 1e3 if k.endswith("_ms") else 1.0) for k in legs} if att else None
    if att:
        res["upload_over_attaching_tick"] = res["attaching_ticks"]["upload_ms"]["median"] / res["attaching_ticks"]["tick_ms"]["median"]
        legs = {k: [v[i] for i in att] for k, v in legs.items()}
    tick_med, up_med = res["border_crossing"]["tick_ms"]["median"], res["border_crossing"]["upload_ms"]["median"]
    res["upload_over_tick"] = up_med / tick_med if tick_med > 0 else None
    kern = np.asarray(legs["kernel_us"], dtype=np.float64); vox = np.asarray(legs["voxels"], dtype=np.float64)
    res["encode_kernel_gb_s_of_9_bytes_a_voxel"] = float(np.median(9.0 * vox / np.maximum(kern, 1e-3) / 1e3))
    res["pool"] = g.grid_pool_stats()
    # the same tick between frames in flight
    periods = {"with_tick": [], "without_tick": [], "with_tick_less_python": []}
    outstanding, lib_ms = [], []
    for k in range(2 * max(4, a.ticks // 2)):
        with_tick = k % 2 == 0
        g.RenderAsync(); g.RenderAsync()
        g.Wait()
        t0 = time.perf_counter()
        g.RenderAsync(); g.RenderAsync()
        python_s = 0.0
        if with_tick:
            t1 = time.perf_counter()
            tick(32.0 if (k // 2) % 2 == 0 else 0.0)
            g.StreamObjects(scene)
            c = g.stream_call_s
            lib = c["attach"] + c["update"] + c["detach"]
            python_s = (time.perf_counter() - t1) - lib          # world slicing and flattening: what a native host does not pay
            lib_ms.append(lib)
            outstanding.append(int(g.flight_info()["frames_outstanding"]))
        g.RenderAsync(); g.RenderAsync()
        g.Wait()
        wall = time.perf_counter() - t0
        periods["with_tick" if with_tick else "without_tick"].append(wall / 4)
        if with_tick:
            periods["with_tick_less_python"].append((wall - python_s) / 4)
    res["frames_in_flight"] = {"frame_period_ms_with_tick_wall": stats(periods["with_tick"]), "frame_period_ms_without_tick": stats(periods["without_tick"]),
                               "frame_period_ms_with_tick_less_python": stats(periods["with_tick_less_python"]),
                               "tick_library_calls_ms": stats(lib_ms),
                               "frames_outstanding_after_tick": int(max(outstanding)) if outstanding else None,
                               "note": "periods are over 4 frames with the tick after the second; 'wall' includes the Python world slicing and flattening of the "
                                       "tick, 'less_python' takes that time off (the two frames queued before the tick run beside it, so this is a lower "
                                       "bound of a native host's period); ycge_scene_attach_grids joins the frames in flight"}
    g.close(); t.close()
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
