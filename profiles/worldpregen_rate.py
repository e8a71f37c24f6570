"""The pregenerated world of BuildMinecraftLike (WorldManager.GenerateAndSaveWorld: 32 x 8 x 32 chunks of 32, seed 0, origin (0, 0)) made
and attached two ways on the same machine:

  * one ycge_scene_generate_world call (the device path): wall time, one warm-up and the median of --runs, a fresh context each; the
    kernel times per stage and the number of anyLeaves passes from ycge_debug_worldpregen_stats;
  * ycge_worldgen_world_cells on the host (one thread), then ycge_scene_attach_grids of the chunks that hold something, in the same order.

Written to profiles/worldpregen_rate.json.

    python profiles/worldpregen_rate.py [--runs 5] [--chunks 32] [--host-runs 1]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "profiles"))
from worldgen_rate import anchor, proto                                   # noqa: E402
from yetanotherconsolegameengine_amd import abi, build                    # noqa: E402
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer     # noqa: E402

S, CHUNKS_Y = 32, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=32, help="chunks_x = chunks_z (the reference: 32)")
    ap.add_argument("--host-runs", type=int, default=1)
    a = ap.parse_args()
    n = a.chunks
    wmin = (-n * S / 2.0, 0.0, -n * S / 2.0)          # the world centred on the origin, as profiles/worldgen_rate.py has it
    world = abi.World(S, CHUNKS_Y, 0, abi.Vec3(*wmin), abi.Vec3(1, 1, 1))
    g, keep = proto()
    L = abi.load_library()
    out = {"build": build.source_hash(), "chunk": S, "chunks": [n, CHUNKS_Y, n], "cells": (n * S) ** 2 * CHUNKS_Y * S, "runs": a.runs}
    wall, stats, idx = [], [], None
    for k in range(a.runs + 1):          # (the first is the warm-up)
        r = RaytraceRenderer(anchor(), 96, 27)
        t0 = time.perf_counter()
        idx = r.GenerateWorld(world, n, n, g)
        wall.append(time.perf_counter() - t0)
        stats.append(r.worldpregen_stats())
        r.close()
        print(f"device run {k}: {1e3 * wall[-1]:.1f} ms {stats[-1]}", flush=True)
    wall, stats = wall[1:], stats[1:]
    out["device"] = {"generate_world_ms_median": 1e3 * statistics.median(wall), "generate_world_ms_all": [1e3 * v for v in wall],
                     "any_leaves_passes": stats[0]["any_leaves_passes"], "resident": int((idx >= 0).sum()),
                     **{k + "_median": statistics.median(s[k] for s in stats) for k in ("fields_us", "any_leaves_us", "occupied_us", "fill_us")}}
    # the way a build without the export has: the host generator, then an attach of the chunks that hold something
    cells = np.zeros((n * S, CHUNKS_Y * S, n * S, 2), np.int32)
    host_s = []
    for _ in range(a.host_runs):
        t0 = time.perf_counter()
        assert L.ycge_worldgen_world_cells(C.byref(world), n, n, 0, 0, cells.ctypes.data_as(C.POINTER(C.c_int32))) == abi.YCGE_OK
        host_s.append(time.perf_counter() - t0)
        print(f"host generator: {host_s[-1]:.2f} s", flush=True)
    t0 = time.perf_counter()
    occ = (cells[..., 0] != 0).reshape(n, S, CHUNKS_Y, S, n, S).any(axis=(1, 3, 5))
    keys = [tuple(int(v) for v in k) for k in np.argwhere(occ)]
    chunks = [np.ascontiguousarray(cells[k[0] * S:(k[0] + 1) * S, k[1] * S:(k[1] + 1) * S, k[2] * S:(k[2] + 1) * S]) for k in keys]
    slice_s = time.perf_counter() - t0          # (AttachChunkFromPreloaded's own slicing, :703-719)
    assert len(keys) == out["device"]["resident"] and (occ == (idx >= 0)).all()
    recs = (abi.Grid * len(keys))()
    for j, k in enumerate(keys):
        C.memmove(C.byref(recs[j]), C.byref(g), C.sizeof(abi.Grid))
        recs[j].nx = recs[j].ny = recs[j].nz = S
        recs[j].min_corner = abi.Vec3(*[wmin[ax] + k[ax] * S for ax in range(3)])
        recs[j].cells = chunks[j].ctypes.data_as(C.POINTER(C.c_int32))
    att = []
    for k in range(min(a.runs, 3)):
        r = RaytraceRenderer(anchor(), 96, 27)
        o = (C.c_int32 * len(keys))()
        t0 = time.perf_counter()
        r._check(L.ycge_scene_attach_grids(r.ctx, recs, len(keys), o))
        att.append(time.perf_counter() - t0)
        r.close()
        print(f"attach run {k}: {1e3 * att[-1]:.1f} ms", flush=True)
    out["host"] = {"world_cells_ms_median": 1e3 * statistics.median(host_s), "world_cells_runs": a.host_runs, "slice_ms": 1e3 * slice_s,
                   "attach_ms_median": 1e3 * statistics.median(att), "world_cells_then_attach_ms": 1e3 * (statistics.median(host_s) + statistics.median(att))}
    out["device_faster_than_host"] = out["device"]["generate_world_ms_median"] < out["host"]["world_cells_then_attach_ms"]
    (ROOT / "profiles" / "worldpregen_rate.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
