"""The world store (ycge_world_store_load / ycge_scene_attach_world_chunks) against the path it replaces: world_file.slice_chunk on the
host and ycge_scene_attach_grids of the slices.

    python profiles/world_store_rate.py [--ticks N] [--small] [--whole-world]     -> profiles/world_store_rate.json

One process, one MI355X, two contexts over the same anchor scene; the two paths alternate (which goes first alternates too) and are warmed.
ATTACHING TICK: profiles/stream_rate.py's world (544 x 256 x 544, chunks of 32, view distance 8): per tick the camera column moves one
chunk along x, back and forth, and the row of 17 x 8 chunk positions that enters is attached (51 hold anything), the row that left is
detached.  Timed per path: the library call alone, and with the host's slicing (the store path has none: its keys are all it prepares).
At x = 32 the entering row is cx = 17, outside the 17-chunk-wide world: every other tick asks for 136 keys and attaches nothing.  As in
profiles/stream_rate.py only the ticks that attached something are measured (`attaching_tick`), and the run goes on until --ticks of them
(16 at least) are in; the others are counted (`empty_ticks`) and summarised apart (`empty_tick`).  Medians over the attaching ticks and each
path's own min-to-p99 spread over them; `condition_met`: the store path's median is not above the attach path's by more than the attach
path's spread.
WHOLE WORLD (--whole-world): the reference's 1024 x 256 x 1024 with S = 32, cells from ycge_scene_generate_world(..., cells_out):
LoadWorld + the attach of all keys against host slicing + ycge_scene_attach_grids of all occupied chunks, fresh contexts, with the load's
split from ycge_debug_world_store_stats.  No threshold.
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


def stats(t, scale=1e3):
    t = np.asarray(t, dtype=np.float64) * scale
    return {"median": float(np.median(t)), "p99": float(np.percentile(t, 99)), "min": float(t.min()), "spread_min_to_p99": float(np.percentile(t, 99) - t.min()),
            "n": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="a 96 x 128 x 96 world, view distance 1, and a 4 x 4 x 4 chunk whole world (a rehearsal of the script, not a measurement)")
    ap.add_argument("--whole-world", action="store_true", help="also the whole-world step (2.1 GB of cells on the host)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "world_store_rate.json"))
    a = ap.parse_args()
    from test_gpu_worldgen import _anchor
    from yetanotherconsolegameengine_amd import abi, build, scenes, world_file as wf
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

    I32P = C.POINTER(C.c_int32)
    chunk = 32
    res = {"what": "the world store against host slices + ycge_scene_attach_grids on one MI355X; profiles/world_store_rate.py", "build": build.source_hash()}

    def proto_for(world, wmin):
        m, t = world[..., 0], world[..., 1]
        assert m.min() >= 0 and m.max() < 64 and t.min() >= 0 and t.max() < 8
        codes = np.flatnonzero(np.bincount((m * 8 + t).ravel(), minlength=512))          # (a count, not a sort: 75 M cells)
        pairs = [(c // 8, c % 8) for c in codes if c // 8 > 0]
        lk = (abi.VoxelLookup * len(pairs))(*[abi.VoxelLookup(int(m), int(t), (int(m) * 3 + int(t)) % 27) for m, t in pairs])
        g = abi.Grid()
        g.lookup, g.n_lookup, g.default_material = C.cast(lk, C.POINTER(abi.VoxelLookup)), len(pairs), -1
        g.wireframe, g.wire_width_fraction, g.wire_max_distance = 1, 0.06, 16.0
        g.voxel_size, g.min_corner = abi.Vec3(1, 1, 1), abi.Vec3(*wmin)
        return g, lk

    def host_attach(r, world, keys, proto, wmin, clock):
        """slice on the host, attach the slices -> indices per key; clock: [slicing seconds, library seconds]"""
        t0 = time.perf_counter()
        parts = [(j, wf.slice_chunk(world, *k, chunk)) for j, k in enumerate(keys)]
        parts = [(j, p) for j, p in parts if p is not None]
        recs = (abi.Grid * max(1, len(parts)))()
        for n, (j, p) in enumerate(parts):
            C.memmove(C.byref(recs[n]), C.byref(proto), C.sizeof(abi.Grid))
            recs[n].nx, recs[n].ny, recs[n].nz = p.shape[:3]
            recs[n].min_corner = abi.Vec3(*[np.float32(wmin[i]) + np.float32(keys[j][i] * chunk) * np.float32(1) for i in range(3)])
            recs[n].cells = p.ctypes.data_as(I32P)
        out = (C.c_int32 * max(1, len(parts)))()
        t1 = time.perf_counter()
        rc = r.L.ycge_scene_attach_grids(r.ctx, recs, len(parts), out)
        t2 = time.perf_counter()
        r._check(rc)
        clock[0] += t1 - t0; clock[1] += t2 - t1
        idx = [-1] * len(keys)
        for n, (j, p) in enumerate(parts):
            idx[j] = int(out[n])
        return idx

    # ---------------------------------------------------------------- the attaching tick
    nx, ny, nz, view = (96, 128, 96, 1) if a.small else (544, 256, 544, 8)
    world = np.ascontiguousarray(scenes.make_voxel_world(nx, ny, nz), np.int32)
    wmin, vox = (-nx // 2, 0.0, -nz // 2), (1.0, 1.0, 1.0)
    chunks_y = ny // chunk
    proto, keep = proto_for(world, wmin)
    H, S = RaytraceRenderer(_anchor(), 160, 90), RaytraceRenderer(_anchor(), 160, 90)
    S.LoadWorld(world, chunk)
    res["tick_world"] = {"dims": [nx, ny, nz], "view_distance_chunks": view, "load": S.world_store_stats(), "load_call_ms": S.stream_call_s["load_world"] * 1e3}
    loaded_h, loaded_s = {}, {}

    def tick_host(x, clock):
        desired = wf.build_desired_set((x, 0.0, 0.0), wmin, vox, chunk, view, chunks_y)
        want = set(desired)
        gone = [loaded_h.pop(k) for k in [k for k in loaded_h if k not in want]]
        cx0, cz0 = wf.center_column((x, 0.0, 0.0), wmin, vox, chunk)
        todo = [k for k in desired if k not in loaded_h]
        todo.sort(key=lambda k: ((k[0] - cx0) ** 2 + (k[2] - cz0) ** 2, k[1]))
        idx = host_attach(H, world, todo, proto, wmin, clock) if todo else []
        loaded_h.update(zip(todo, idx))
        return todo, idx, [i for i in gone if i >= 0]

    def detach(r, idx):
        if idx:
            arr = (C.c_int32 * len(idx))(*idx)
            r._check(r.L.ycge_scene_detach_grids(r.ctx, arr, len(idx)))

    legs = {k: [] for k in ("attach_lib_ms", "attach_with_slicing_ms", "store_lib_ms", "store_with_python_ms", "slice_kernel_us", "chunks_in", "keys", "raw_mb",
                            "attach_stage_us", "attach_h2d_us", "attach_kernel_us", "store_stage_us", "store_h2d_us", "store_kernel_us")}
    k = -2
    while sum(1 for v in legs["chunks_in"] if v > 0) < max(16, a.ticks) and k < 8 * max(16, a.ticks):
        k += 1
        x = 0.0 if k < 0 or k % 2 == 1 else 32.0          # (k = -1: the first view, not a tick)
        for leg in (("host", "store") if (k // 2) % 2 == 0 else ("store", "host")):          # (by pairs of ticks: the attaching ticks are every other one)
            if leg == "host":
                clock = [0.0, 0.0]
                todo, idx_h, gone = tick_host(x, clock)
                detach(H, gone)
                hp = H.grid_pool_stats()
            else:
                t0 = time.perf_counter()
                added, removed, gone = wf.stream_resident(S, proto, (x, 0.0, 0.0), chunk, view, chunks_y, loaded_s)
                wall_s = time.perf_counter() - t0
                lib_s = S.stream_call_s["attach_world"] if added else 0.0
                detach(S, gone)
                sp, ws = S.grid_pool_stats(), S.world_store_stats()
        assert [loaded_s[key] >= 0 for key in todo] == [i >= 0 for i in idx_h]
        if k < a.warmup:
            continue
        n_in = sum(i >= 0 for i in idx_h)
        for name, v in (("attach_lib_ms", clock[1]), ("attach_with_slicing_ms", clock[0] + clock[1]), ("store_lib_ms", lib_s), ("store_with_python_ms", wall_s)):
            legs[name].append(v)
        for name, v in (("slice_kernel_us", ws["last_slice_us"]), ("chunks_in", n_in), ("keys", len(todo)), ("raw_mb", n_in * chunk ** 3 * 8 / 1e6),
                        ("attach_stage_us", hp["last_stage_us"]), ("attach_h2d_us", hp["last_h2d_us"]), ("attach_kernel_us", hp["last_kernel_us"]),
                        ("store_stage_us", sp["last_stage_us"]), ("store_h2d_us", sp["last_h2d_us"]), ("store_kernel_us", sp["last_kernel_us"])):
            legs[name].append(v)
    att = [i for i, v in enumerate(legs["chunks_in"]) if v > 0]          # the ticks that attached something
    rest = [i for i, v in enumerate(legs["chunks_in"]) if v == 0]
    assert len(att) >= 16, len(att)
    t = {k: stats([v[i] for i in att], 1e3 if k.endswith("_ms") else 1.0) for k, v in legs.items()}
    res["empty_ticks"] = len(rest)
    res["empty_tick"] = {k: stats([v[i] for i in rest]) for k, v in legs.items() if k.endswith("_ms")} if rest else None
    t["condition_met"] = bool(t["store_lib_ms"]["median"] <= t["attach_lib_ms"]["median"] + t["attach_lib_ms"]["spread_min_to_p99"])
    t["store_minus_attach_median_ms"] = t["store_lib_ms"]["median"] - t["attach_lib_ms"]["median"]
    res["attaching_tick"] = t
    H.close(); S.close()
    del world

    # ---------------------------------------------------------------- the whole world
    if a.whole_world:
        cx, cy, cz = (4, 4, 4) if a.small else (32, 8, 32)
        gw = abi.World(chunk, cy, 0, abi.Vec3(-cx * chunk / 2.0, 0.0, -cz * chunk / 2.0), abi.Vec3(1, 1, 1))
        wmin = (gw.world_min.x, gw.world_min.y, gw.world_min.z)
        G = RaytraceRenderer(_anchor(), 160, 90)
        pairs = [(m, k) for m in range(1, 9) for k in range(3)]
        lk = (abi.VoxelLookup * len(pairs))(*[abi.VoxelLookup(m, k, (m * 3 + k) % 27) for m, k in pairs])
        proto = abi.Grid()
        proto.lookup, proto.n_lookup, proto.default_material = C.cast(lk, C.POINTER(abi.VoxelLookup)), len(pairs), -1
        proto.wireframe, proto.wire_width_fraction, proto.wire_max_distance = 1, 0.06, 16.0
        proto.voxel_size, proto.min_corner = abi.Vec3(1, 1, 1), abi.Vec3(*wmin)
        gen_idx, cells = G.GenerateWorld(gw, cx, cz, proto, want_cells=True)
        G.close()
        keys = [(x, y, z) for x in range(cx) for y in range(cy) for z in range(cz)]
        runs = {"store": [], "host": []}
        for rep in range(2):          # (the first is the warm-up: the runtime's first allocations of this size)
            for leg in (("store", "host") if rep % 2 == 0 else ("host", "store")):
                r = RaytraceRenderer(_anchor(), 160, 90)
                if leg == "store":
                    t0 = time.perf_counter()
                    r.LoadWorld(cells, chunk)
                    t1 = time.perf_counter()
                    idx = r.AttachWorldChunks(keys, proto)
                    t2 = time.perf_counter()
                    ws = r.world_store_stats()
                    runs[leg].append({"load_ms": (t1 - t0) * 1e3, "attach_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3, "load_split": ws, "slice_kernel_us": ws["last_slice_us"]})
                else:
                    clock = [0.0, 0.0]
                    idx = host_attach(r, cells, keys, proto, wmin, clock)
                    runs[leg].append({"slicing_ms": clock[0] * 1e3, "attach_ms": clock[1] * 1e3, "total_ms": (clock[0] + clock[1]) * 1e3})
                assert (np.asarray(idx, np.int32).reshape(cx, cy, cz) == gen_idx).all()
                runs[leg][-1]["resident"] = r.grid_pool_stats()["resident"]
                r.close()
        res["whole_world"] = {"dims": [cx * chunk, cy * chunk, cz * chunk], "chunk": chunk, "warm_up": {k: v[0] for k, v in runs.items()}, "measured": {k: v[1] for k, v in runs.items()},
                              "note": "one measured run per path after one warm-up run; the host path's slicing is numpy's (world_file.slice_chunk)"}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
