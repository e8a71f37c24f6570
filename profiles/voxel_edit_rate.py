"""Voxel edits on the device (ycge_scene_edit_voxels, ycge_world_store_edit) against what a host does without them: keep the chunk's raw cells,
edit the copy, attach the whole chunk again (ycge_scene_attach_grids), point the object at the new grid (ycge_scene_update_objects) and
give the old one back (ycge_scene_detach_grids - in this order: a grid that an object holds cannot be detached first).

    python profiles/voxel_edit_rate.py [--reps N] [--small]     -> profiles/voxel_edit_rate.json

One process, one MI355X, the config-5 streamed world (544 x 256 x 544, chunks of 32, view distance 8; --small: 96 x 128 x 96, view 1 - a
rehearsal of the script, not a measurement).  Three cases, each a toggle so that every repetition changes cells: one cell inside its
chunk's solid box; one cell above everything in its chunk (the box changes: the objects are installed again); a radius-5 sphere as
x-runs, centred on a chunk border.  For every case the two paths ALTERNATE in one process on the same context - repetition k by the
edit call, k + 1 by the three calls - and the same ops go to the world store (ycge_world_store_edit).  Timed: the library calls alone
(a host clock around calls that end in a device synchronise); reported: medians with the min-to-p99 spread.  No threshold anywhere."""
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


def stats(t, scale=1e3):
    t = np.asarray(t, dtype=np.float64) * scale
    return {"median": float(np.median(t)), "p99": float(np.percentile(t, 99)), "min": float(t.min()), "spread_min_to_p99": float(np.percentile(t, 99) - t.min()), "n": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "voxel_edit_rate.json"))
    a = ap.parse_args()
    from voxel_edit_restatement import apply_ops, op
    from yetanotherconsolegameengine_amd import abi, build, scenes, world_file
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import AmbientLight, Scene, flatten, grid_record, vec3

    nx, ny, nz, view = (96, 128, 96, 1) if a.small else (544, 256, 544, 8)
    S = 32
    world = scenes.make_voxel_world(nx, ny, nz)
    wmin, voxel = (-nx // 2, 0.0, -nz // 2), (1.0, 1.0, 1.0)
    scene = Scene()
    scene.IsVolumeScene = True
    scene.Ambient = AmbientLight(vec3(1, 1, 1), 0.0)
    lights, top, bottom = scenes.sun_moon_lights(0.5)
    scene.Lights.extend(lights)
    scene.BackgroundTop, scene.BackgroundBottom = top, bottom
    loaded = {}
    eye_y = float(int(np.nonzero(world[nx // 2, :, nz // 2, 0])[0].max()) + 1) + 1.8
    empty = flatten(scene)
    w, h, ss = (160, 90, 1) if a.small else (1920, 540, 2)
    g = RaytraceRenderer(empty, w, h, 45.0, ss)
    world_file.stream_view(scene, world, (0.0, eye_y, 0.0), wmin, voxel, S, view, scenes.VoxelMaterialLookup, loaded)
    g.StreamObjects(scene)                    # every chunk attached: encoded on the device, as a streaming host's are
    g.SetCamera((0.0, eye_y, 0.0), 0.0, -0.2)
    g.TryFlipAndBlit()
    g.LoadWorld(world, S)
    L = g.L

    # the chunk under the camera whose cells hold the surface, and the one beside it in x
    cx, cz = (nx // 2) // S, (nz // 2) // S
    x0, z0 = cx * S + 7, cz * S + 9
    hs = int(np.nonzero(world[x0, :, z0, 0] > 0)[0].max())          # the surface cell of that column
    cy = hs // S
    part = world[cx * S:(cx + 1) * S, cy * S:(cy + 1) * S, cz * S:(cz + 1) * S, 0] > 0
    free_y = cy * S + int(np.nonzero(part.any(axis=(0, 2)))[0].max()) + 1          # the first plane of the chunk above all its cells
    pair = tuple(int(v) for v in world[x0, hs, z0])
    if free_y >= (cy + 1) * S or hs - 3 < cy * S:
        sys.exit("the chunk under the camera has no free plane or no depth below the surface: choose another column")
    sphere = []
    c = np.array([(cx + 1) * S, hs - 8, z0])          # centred on the border between chunk cx and cx + 1, under the surface
    for dy in range(-5, 6):
        for dz in range(-5, 6):
            r2 = 25 - dy * dy - dz * dz
            if r2 >= 0:
                rx = int(np.sqrt(r2))
                sphere.append(((c[0] - rx, c[1] + dy, c[2] + dz), (c[0] + rx, c[1] + dy, c[2] + dz)))
    cases = {
        "one cell inside the box": [((x0, hs - 2, z0), (x0, hs - 2, z0))],
        "one cell that changes the box": [((x0, free_y, z0), (x0, free_y, z0))],
        "radius-5 sphere across a chunk border": sphere,
    }
    keep = []

    def edit_path(world_ops):
        local = world_file.clip_ops_to_chunks(world_ops, [k for k in loaded], S)
        rows = []
        for key, boxes in local.items():
            vg = loaded[key]
            mine = [[g.flat._grid_index[id(vg)], *b] for b in boxes]
            vg.Cells = apply_ops(vg.Cells, mine)
            rows += mine
        info = g.EditVoxels(rows)
        return g.stream_call_s["edit"], info

    def host_path(world_ops):
        """the three calls, for every chunk the ops touch"""
        local = world_file.clip_ops_to_chunks(world_ops, [k for k in loaded], S)
        total = 0.0
        for key, boxes in local.items():
            vg = loaded[key]
            old = g.flat._grid_index[id(vg)]
            vg.Cells = apply_ops(vg.Cells, [[0, *b] for b in boxes])
            rec = (abi.Grid * 1)(grid_record(vg, lambda m: g.flat._mat_index[id(m)], keep))
            out = (C.c_int32 * 1)(-1)
            prims, n = C.cast(g.flat.prims, C.POINTER(abi.Prim)), g.flat.struct.n_prims
            at = next(i for i in range(n) if prims[i].type == abi.PRIM_VOLUME_GRID and prims[i].ref == old)
            t0 = time.perf_counter()
            rc = L.ycge_scene_attach_grids(g.ctx, rec, 1, out)
            prims[at].ref = out[0]
            rc = rc or L.ycge_scene_update_objects(g.ctx, prims, n)
            rc = rc or L.ycge_scene_detach_grids(g.ctx, (C.c_int32 * 1)(old), 1)
            total += time.perf_counter() - t0
            g._check(rc)
            g.flat._grid_index[id(vg)] = int(out[0])
            del keep[:]
        return total

    res = {"what": "ycge_scene_edit_voxels / ycge_world_store_edit against attach + update_objects + detach of the edited chunk on one MI355X; profiles/voxel_edit_rate.py",
           "build": build.source_hash(), "world": [nx, ny, nz], "view_distance_chunks": view, "resident_grids": len(loaded), "small": bool(a.small), "cases": {}}
    for name, boxes in cases.items():
        legs = {"edit_ms": [], "host_ms": [], "store_ms": []}
        start_solid = bool(world[boxes[0][0]][0] > 0)
        fill = tuple(int(v) for v in world[tuple(c)]) if len(boxes) > 1 else pair
        for key in world_file.clip_ops_to_chunks([op(lo, hi, fill) for lo, hi in boxes], list(loaded), S):          # (an attached chunk's lookup table holds the pairs of its own cells)
            if fill[0] <= 0 or not ((loaded[key].Cells[..., 0] == fill[0]) & (loaded[key].Cells[..., 1] == fill[1])).any():
                sys.exit(f"chunk {key} does not hold the pair {fill}: choose another column")
        info = None
        for k in range(2 * (a.warmup + a.reps)):
            value = (0, 0) if ((k // 2) % 2 == 0) == start_solid else fill          # a toggle: the edit path (even k) always changes cells, the host path repeats it
            world_ops = [op(lo, hi, value) for lo, hi in boxes]
            if k % 2 == 0:
                t, info_k = edit_path(world_ops)
                info = info_k if k >= 2 * a.warmup and info is None else info
                g.EditWorldCells(world_ops)
                if k >= 2 * a.warmup:
                    legs["edit_ms"].append(t); legs["store_ms"].append(g.stream_call_s["edit_world"])
            else:
                t = host_path(world_ops)
                if k >= 2 * a.warmup:
                    legs["host_ms"].append(t)
        g.TryFlipAndBlit()
        entry = {k: stats(v) for k, v in legs.items()}
        entry["ops"] = len(boxes); entry["info_of_one_edit"] = info
        entry["host_over_edit"] = entry["host_ms"]["median"] / entry["edit_ms"]["median"]
        res["cases"][name] = entry
        print(name, json.dumps(entry))
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    g.close()


if __name__ == "__main__":
    main()
