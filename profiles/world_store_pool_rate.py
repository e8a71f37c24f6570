"""Edits on a fields-form world store through its pool of materialised chunks (ycge_world_store_reserve_edits) against a cells-form
store, and what the pool costs a store that does not use it.

    python profiles/world_store_pool_rate.py [--parent-lib PATH] [--reps N] [--ticks N] [--small]     -> profiles/world_store_pool_rate.json

One process, one MI355X, the reference's 32 x 8 x 32 chunks of 32 at origin (0, 0) (--small: 4 x 4 x 4 chunks, a rehearsal of the script,
not a measurement).  Every timed step is warmed, repeated, and reported as its median with its own min-to-p99 spread; the stores of a
leg alternate inside one process.
DIG TICK: a one-cell ycge_world_store_edit (the library call) on a fields store with a pool of 256 slots - the chunk pooled already,
and the chunk not pooled yet (ycge_world_store_revert_chunks before every timed call, untimed: k_wp_fill makes the chunk again) -
against the same op on a cells-form store.
STREAMING TICK: the tick of profiles/world_store_generate_rate.py - view distance 8, the camera column moves one chunk along x, back
and forth, 136 keys enter - on a cells store, a fields store without a pool, and fields stores with 0, 8 and 68 of the occupied keys
of each entering row pooled (a solid cell written into each; the cells store takes the same ops).  Timed: the library call
(ycge_scene_attach_world_chunks).  All must agree on how many keys took a grid.
AGAINST THE PARENT: with --parent-lib, the parent commit's library (built elsewhere from the parent's sources) is loaded beside the
product's; two parent contexts with an unpooled fields store run the same ticks, alternated with the others.  The parent's spread
against itself is the yardstick: the product's unpooled fields store must not be slower than the parent by more than it.  Without
--parent-lib this part is "not measured".
RESIDENT BYTES: the fields plus a pool of 256 slots against the cells form, a device.
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

POOL_EXPORTS = ("ycge_world_store_reserve_edits", "ycge_world_store_edit_slots", "ycge_world_store_revert_chunks")


def stats(t, scale=1e3):
    t = np.asarray(t, dtype=np.float64) * scale
    return {"median": float(np.median(t)), "p99": float(np.percentile(t, 99)), "min": float(t.min()), "spread_min_to_p99": float(np.percentile(t, 99) - t.min()),
            "n": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--small", action="store_true", help="4 x 4 x 4 chunks and view distance 1 (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "world_store_pool_rate.json"))
    a = ap.parse_args()
    from test_gpu_worldgen import _anchor
    from yetanotherconsolegameengine_amd import abi, build, world_file as wf
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer

    S = 32
    cx, cy, cz, view, slots = (4, 4, 4, 1, 16) if a.small else (32, 8, 32, 8, 256)
    gw = abi.World(S, cy, 0, abi.Vec3(-cx * S / 2.0, 0.0, -cz * S / 2.0), abi.Vec3(1, 1, 1))
    wmin, vox = (gw.world_min.x, gw.world_min.y, gw.world_min.z), (1.0, 1.0, 1.0)
    res = {"what": "a fields store with a pool of materialised chunks against a cells store on one MI355X; profiles/world_store_pool_rate.py",
           "build": build.source_hash(), "dims": [cx * S, cy * S, cz * S], "chunk": S, "pool_slots": slots, "small": bool(a.small)}
    pairs = [(m, k) for m in range(1, 9) for k in range(3)]
    lk = (abi.VoxelLookup * len(pairs))(*[abi.VoxelLookup(m, k, (m * 3 + k) % 27) for m, k in pairs])
    proto = abi.Grid()
    proto.lookup, proto.n_lookup, proto.default_material = C.cast(lk, C.POINTER(abi.VoxelLookup)), len(pairs), -1
    proto.wireframe, proto.wire_width_fraction, proto.wire_max_distance = 1, 0.06, 16.0
    proto.voxel_size, proto.min_corner = abi.Vec3(1, 1, 1), abi.Vec3(*wmin)

    def make(form, pool=None, lib=None):
        r = RaytraceRenderer(_anchor(), 160, 90, lib=lib)
        r.GenerateWorldStore(gw, cx, cz, form=form)
        if pool is not None:
            r.ReserveWorldEdits(pool)
        return r

    # ---------------------------------------------------------------- the dig tick
    Fp, Cs = make("fields", slots), make("cells")
    occ = Cs.WorldInfo()[2]
    dig_key = tuple(int(v) for v in np.argwhere(occ)[len(np.argwhere(occ)) // 2])
    cell = tuple(k * S + 5 for k in dig_key)
    legs = {"fields_chunk_pooled": [], "fields_chunk_not_pooled": [], "cells": []}
    Fp.EditWorldCells([[0, *cell, *cell, 1, 0]])          # (the chunk takes its slot)
    for rep in range(-a.warmup, a.reps):
        op = [[0, *cell, *cell, 1 + rep % 2, 0]]
        order = list(legs) if rep % 2 == 0 else list(legs)[::-1]
        for leg in order:
            r = Cs if leg == "cells" else Fp
            if leg == "fields_chunk_not_pooled":
                r.RevertWorldChunks([dig_key])
            r.EditWorldCells(op)
            if rep >= 0:
                legs[leg].append(r.stream_call_s["edit_world"])
    assert Fp.WorldEditSlots() == (slots, 1)
    res["dig_tick"] = {k + "_ms": stats(v) for k, v in legs.items()}
    st = Fp.world_store_stats()
    res["resident_bytes"] = {"fields": st["store_bytes"], "pool_of_%d_slots" % slots: st["edit_pool_bytes"], "fields_plus_pool": st["store_bytes"] + st["edit_pool_bytes"],
                             "cells": Cs.world_store_stats()["store_bytes"]}
    Fp.close()

    # ---------------------------------------------------------------- the streaming tick
    xs = (0.0, 32.0)
    desired = [set(wf.build_desired_set((x, 0.0, 0.0), wmin, vox, S, view, cy)) for x in xs]
    inside = lambda k: all(0 <= k[i] < occ.shape[i] for i in range(3))
    rows = [sorted(k for k in desired[1] - desired[0] if inside(k) and occ[k]), sorted(k for k in desired[0] - desired[1] if inside(k) and occ[k])]          # the occupied keys that enter, either way
    res["entering_occupied_keys"] = [len(r) for r in rows]

    def pooled_ops(n):
        return [[0, *(k * S for k in key), *(k * S for k in key), 1, 0] for row in rows for key in row[:n]]

    stores = {"cells": Cs, "fields_unpooled": make("fields")}
    counts = (0, 2, 3) if a.small else (0, 8, 68)
    for n in counts:
        r = make("fields", slots)
        if n:
            r.EditWorldCells(pooled_ops(n))
        stores["fields_%d_pooled" % n] = r
    Cs.EditWorldCells(pooled_ops(max(counts)))          # (occupied chunks stay occupied: every store attaches the same keys)
    if a.parent_lib:
        P = abi.bind(C.CDLL(str(a.parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n not in POOL_EXPORTS])
        assert not hasattr(P, POOL_EXPORTS[0]), "the parent's library is expected to lack the export"
        stores["parent A"], stores["parent B"] = make("fields", lib=P), make("fields", lib=P)
    res["pooled_slots_in_use"] = {name: r.WorldEditSlots()[1] for name, r in stores.items() if not name.startswith("parent")}
    loaded = {k: {} for k in stores}
    tick = {k: {"lib_ms": [], "chunks_in": [], "keys": []} for k in stores}
    names = list(stores)
    for k in range(-1 - a.warmup, a.ticks):          # (the first: the whole view, not a tick)
        x = xs[(k + 1 + a.warmup) % 2]
        got = {}
        for name in names[k % len(names):] + names[:k % len(names)]:
            r = stores[name]
            added, removed, gone = wf.stream_resident(r, proto, (x, 0.0, 0.0), S, view, cy, loaded[name])
            r.DetachGrids(gone)
            got[name] = sum(loaded[name][key] >= 0 for key in added)
            if k >= 0:
                t = tick[name]
                t["lib_ms"].append(r.stream_call_s["attach_world"] if added else 0.0); t["chunks_in"].append(got[name]); t["keys"].append(len(added))
        assert len(set(got.values())) == 1, got
    res["streaming_tick"] = {name: {"lib_ms": stats(t["lib_ms"]), "chunks_in": stats(t["chunks_in"], 1.0), "keys": stats(t["keys"], 1.0)} for name, t in tick.items()}
    res["streaming_tick"]["view_distance_chunks"] = view
    if a.parent_lib:
        parent = np.asarray(tick["parent A"]["lib_ms"] + tick["parent B"]["lib_ms"]) * 1e3
        pa, pb = np.median(tick["parent A"]["lib_ms"]) * 1e3, np.median(tick["parent B"]["lib_ms"]) * 1e3
        mine = float(np.median(tick["fields_unpooled"]["lib_ms"]) * 1e3)
        spread = float(max(abs(pa - pb), np.percentile(parent, 99) - parent.min()))
        res["unpooled_against_parent"] = {"product_median_ms": mine, "parent_median_ms": float(np.median(parent)), "parent_A_median_ms": float(pa), "parent_B_median_ms": float(pb),
                                          "parent_spread_ms": spread, "product_minus_parent_ms": mine - float(np.median(parent)),
                                          "not_slower_by_more_than_the_parents_spread": bool(mine - float(np.median(parent)) <= spread)}
    else:
        res["unpooled_against_parent"] = "not measured"
    for r in stores.values():
        r.close()
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
