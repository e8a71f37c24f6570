"""A world store whose source is the generator (ycge_world_store_generate, both forms) against the path it replaces: the host generator
ycge_worldgen_world_cells followed by ycge_world_store_load.

    python profiles/world_store_generate_rate.py [--reps N] [--ticks N] [--small]     -> profiles/world_store_generate_rate.json

One process, one MI355X, the reference's 32 x 8 x 32 chunks of 32 at origin (0, 0) (--small: 4 x 4 x 4 chunks, a rehearsal of the script,
not a measurement).  Every timed step is warmed once, repeated, and reported as its median with its own min-to-p99 spread.
GENERATE: GenerateWorldStore in the FIELDS and the CELLS form (the library call, and its split from ycge_debug_world_store_generate_stats),
alternated, against LoadWorld of the host generator's cells; the host generator itself runs ONCE (seconds of one CPU thread).
STREAMING TICK: three contexts over the same anchor scene - a fields store, a generated cells store, a loaded store - and the tick of
profiles/world_store_rate.py: view distance 8, the camera column moves one chunk along x, back and forth, so that a row of 17 x 8 chunk
positions enters and one leaves.  The order of the three alternates tick by tick; timed: the library call (ycge_scene_attach_world_chunks)
and the fill / slice kernels' own time.  The three must agree on which keys took a grid.
SAVE: world_file.save_resident of the whole world from the fields store and from the cells store (64 MiB slabs) against
pregen_world(path=...) = the host generator plus write_vg01; the files' bytes must be equal.  The file system's share is in all of them.
No threshold anywhere: the numbers go into README.md's row as they come.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import tempfile
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="4 x 4 x 4 chunks and view distance 1 (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "world_store_generate_rate.json"))
    a = ap.parse_args()
    from test_gpu_worldgen import _anchor
    from yetanotherconsolegameengine_amd import abi, build, world_file as wf
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

    S = 32
    cx, cy, cz, view = (4, 4, 4, 1) if a.small else (32, 8, 32, 8)
    gw = abi.World(S, cy, 0, abi.Vec3(-cx * S / 2.0, 0.0, -cz * S / 2.0), abi.Vec3(1, 1, 1))
    dims = (cx * S, cy * S, cz * S)
    res = {"what": "ycge_world_store_generate against ycge_worldgen_world_cells + ycge_world_store_load on one MI355X; profiles/world_store_generate_rate.py",
           "build": build.source_hash(), "dims": list(dims), "chunk": S, "small": bool(a.small)}
    pairs = [(m, k) for m in range(1, 9) for k in range(3)]
    lk = (abi.VoxelLookup * len(pairs))(*[abi.VoxelLookup(m, k, (m * 3 + k) % 27) for m, k in pairs])
    proto = abi.Grid()
    proto.lookup, proto.n_lookup, proto.default_material = C.cast(lk, C.POINTER(abi.VoxelLookup)), len(pairs), -1
    proto.wireframe, proto.wire_width_fraction, proto.wire_max_distance = 1, 0.06, 16.0
    proto.voxel_size, proto.min_corner = abi.Vec3(1, 1, 1), abi.Vec3(gw.world_min.x, gw.world_min.y, gw.world_min.z)

    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        # ---------------------------------------------------------------- the host generator, once; its file
        L = abi.load_library()
        cells = np.zeros(dims + (2,), np.int32)
        t0 = time.perf_counter()
        rc = L.ycge_worldgen_world_cells(C.byref(gw), cx, cz, 0, 0, cells.ctypes.data_as(C.POINTER(C.c_int32)))
        t1 = time.perf_counter()
        assert rc == 0
        wf.write_vg01(td / "host.vg", cells)
        t2 = time.perf_counter()
        res["host"] = {"generator_ms": (t1 - t0) * 1e3, "write_vg01_ms": (t2 - t1) * 1e3, "pregen_world_with_path_ms": (t2 - t0) * 1e3, "runs": 1}

        # ---------------------------------------------------------------- generate
        F, Cs, Ld = (RaytraceRenderer(_anchor(), 160, 90) for _ in range(3))
        legs = {"fields": [], "cells": [], "load": []}
        split = {"fields": [], "cells": []}
        for rep in range(-1, a.reps):          # (-1: the warm-up)
            order = ("fields", "cells", "load") if rep % 2 == 0 else ("load", "cells", "fields")
            for leg in order:
                if leg == "load":
                    Ld.LoadWorld(cells, S)
                    s = Ld.stream_call_s["load_world"]
                else:
                    r = F if leg == "fields" else Cs
                    r.GenerateWorldStore(gw, cx, cz, form=leg)
                    s = r.stream_call_s["generate_world_store"]
                    if rep >= 0:
                        split[leg].append(r.world_store_generate_stats())
                if rep >= 0:
                    legs[leg].append(s)
        res["generate"] = {"fields_ms": stats(legs["fields"]), "cells_ms": stats(legs["cells"]), "load_of_host_cells_ms": stats(legs["load"]),
                           "host_generator_plus_load_ms": res["host"]["generator_ms"] + stats(legs["load"])["median"],
                           "fields_split_us": {k: stats([d[k] for d in split["fields"]], 1.0) for k in ("fields_us", "any_leaves_us", "occupied_us")},
                           "cells_split_us": {k: stats([d[k] for d in split["cells"]], 1.0) for k in ("fields_us", "any_leaves_us", "occupied_us", "planes_us")},
                           "any_leaves_passes": split["fields"][0]["any_leaves_passes"], "plane_slabs": split["cells"][0]["plane_slabs"],
                           "store_bytes": {"fields": F.world_store_stats()["store_bytes"], "cells": Cs.world_store_stats()["store_bytes"], "loaded": Ld.world_store_stats()["store_bytes"]}}
        assert F.WorldInfo()[2].tobytes() == Cs.WorldInfo()[2].tobytes() == Ld.WorldInfo()[2].tobytes()

        # ---------------------------------------------------------------- the streaming tick
        stores = {"fields": F, "cells": Cs, "loaded": Ld}
        loaded = {k: {} for k in stores}
        tick = {k: {"lib_ms": [], "kernel_us": [], "chunks_in": [], "keys": []} for k in stores}
        names = list(stores)
        for k in range(-1 - a.warmup, a.ticks):          # (the first: the whole view, not a tick)
            x = 0.0 if (k + 1 + a.warmup) % 2 == 0 else 32.0
            got = {}
            for name in names[k % 3:] + names[:k % 3]:
                r = stores[name]
                added, removed, gone = wf.stream_resident(r, proto, (x, 0.0, 0.0), S, view, cy, loaded[name])
                r.DetachGrids(gone)
                got[name] = [loaded[name][key] >= 0 for key in added]
                if k >= 0:
                    t = tick[name]
                    t["lib_ms"].append(r.stream_call_s["attach_world"] if added else 0.0); t["kernel_us"].append(r.world_store_stats()["last_slice_us"])
                    t["chunks_in"].append(sum(got[name])); t["keys"].append(len(added))
            assert got["fields"] == got["cells"] == got["loaded"]
        res["streaming_tick"] = {name: {"lib_ms": stats(t["lib_ms"]), "kernel_us": stats(t["kernel_us"], 1.0), "chunks_in": stats(t["chunks_in"], 1.0), "keys": stats(t["keys"], 1.0)}
                                 for name, t in tick.items()}
        res["streaming_tick"]["view_distance_chunks"] = view
        Ld.close()
        del cells

        # ---------------------------------------------------------------- save
        save = {}
        want = (td / "host.vg").read_bytes() if a.small else None
        for name, r in (("fields", F), ("cells", Cs), ("fields", F), ("cells", Cs)):          # (the first of each: the warm-up)
            t0 = time.perf_counter()
            wf.save_resident(r, td / "got.vg")
            save.setdefault(name, []).append(time.perf_counter() - t0)
        same = True
        with open(td / "got.vg", "rb") as fa, open(td / "host.vg", "rb") as fb:          # (compared in pieces: neither file is read whole)
            while True:
                ba, bb = fa.read(64 << 20), fb.read(64 << 20)
                same = same and ba == bb
                if not ba and not bb:
                    break
        assert same and (want is None or (td / "got.vg").read_bytes() == want)
        res["save"] = {"save_resident_fields_ms": save["fields"][1] * 1e3, "save_resident_cells_ms": save["cells"][1] * 1e3, "pregen_world_with_path_ms": res["host"]["pregen_world_with_path_ms"],
                       "files_equal": bool(same), "note": "one measured run each after one warm-up run; the file system's share is in all three"}
        F.close(); Cs.close()
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
