"""Mesh BVH build at ycge_scene_upload: the device-side builder (csrc/ycge_mesh_bvh_build.hip) against the host builder it replaces.

    python profiles/mesh_build_rate.py [--runs N]     -> profiles/mesh_build_rate.json

One process, one MI355X, three contexts of the same geometry: one made under YCGE_MESH_BVH_HOST (the host builder: the path before the
device builder existed), one under YCGE_MESH_BVH_DEVICE_MIN=1 and YCGE_MESH_EMIT_HOST=1 (the device builder with the host's
emit_mesh_records and append_treelets behind it: the path before csrc/ycge_mesh_emit.hip existed, the yardstick of the device emit), one
under YCGE_MESH_BVH_DEVICE_MIN=1 and YCGE_MESH_EMIT_DEVICE_MIN=1 (tree, records and treelets on the device).  Per mesh - 1 k, 4 k, 16 k and 250 k triangles (prefixes of config 4's
mesh), the bunny, config 4's whole mesh - the three legs alternate inside the run: one warm-up upload each, then the median of --runs
timed ycge_scene_upload calls each (host clock around the call, which ends synchronised).  Beside the whole upload:
  * the host builder alone (ycge_host_build_mesh) and the device build alone as ycge_debug_mesh_bvh_stats reports it (items kernel to the
    tree in host memory);
  * the split of the device upload: build as above; emit_mesh_records and append_treelets timed on the host through their hooks
    (ycge_host_mesh_arena - ycge_host_build_mesh, ycge_host_mesh_arena_treelets - ycge_host_mesh_arena: both are host code that the
    upload runs unchanged); `copies_and_rest` is what remains of the upload (the triangles' way to the device, install_scene's copies);
  * `upload_device_emit_ms` and its split: build as above; layout + records and treelets as ycge_debug_device_mesh_arena times them
    (each with its wait); `copies_and_rest` is what remains (the triangles' way up, the tree's way back, install_scene).
`device_emit_no_slower` says, per row, whether the device emit upload is no slower than the host emit upload of this run - required at
every size from YCGE_MESH_EMIT_DEVICE_MIN's default on, where it is what an upload does; that default (csrc/ycge_ctx.h) is
`device_emit_crossover_triangles`, the smallest measured count from which on it holds.
`crossover` is the smallest measured count from which on the device upload is no slower than the host upload: the default of
YCGE_MESH_BVH_DEVICE_MIN (csrc/ycge_device.h) is taken from it.
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


def med(t):
    return float(np.median(np.asarray(t, dtype=np.float64)) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mesh_build_rate.json"))
    a = ap.parse_args()
    from yetanotherconsolegameengine_amd import abi, build, scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import AmbientLight, Material, Mesh, PointLight, Scene, flatten, vec3, ZERO

    build.build_library()
    L = abi.load_library()
    big = next(ob.Triangles for ob in scenes.config_scene(4)[0].Objects if isinstance(ob, Mesh))
    bunny = next(ob.Triangles for ob in scenes.config_scene(3)[0].Objects if isinstance(ob, Mesh))
    meshes = [("1k", big[:1000]), ("4k", big[:4000]), ("16k", big[:16000]), ("bunny", bunny), ("250k", big[:250000]), ("config 4", big)]

    def scene_of(tris):
        s = Scene()
        s.Ambient = AmbientLight(vec3(1, 1, 1), 0.3)
        s.Add(Mesh(np.ascontiguousarray(tris, np.float32), Material(vec3(0.7, 0.7, 0.7), 0.1, 0.0, ZERO)))
        s.Lights.append(PointLight(vec3(0, 5, 0), vec3(1, 1, 1), 60.0))
        return s

    def context(env):
        for k in ("YCGE_MESH_BVH_HOST", "YCGE_MESH_BVH_DEVICE_MIN", "YCGE_MESH_EMIT_HOST", "YCGE_MESH_EMIT_DEVICE_MIN"):
            os.environ.pop(k, None)
        os.environ.update(env)
        r = RaytraceRenderer(flatten(scene_of(big[:16])), 160, 90, 45.0, 1)       # (the knobs are read when the context is made)
        for k in env:
            os.environ.pop(k, None)
        return r

    host_ctx, dev_ctx = context({"YCGE_MESH_BVH_HOST": "1"}), context({"YCGE_MESH_BVH_DEVICE_MIN": "1", "YCGE_MESH_EMIT_HOST": "1"})
    emit_ctx = context({"YCGE_MESH_BVH_DEVICE_MIN": "1", "YCGE_MESH_EMIT_DEVICE_MIN": "1"})
    dev_arena = L.ycge_debug_device_mesh_arena
    dev_arena.restype, dev_arena.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_device_mesh_arena"]
    for name in ("ycge_host_build_mesh", "ycge_host_mesh_arena", "ycge_host_mesh_arena_treelets"):
        getattr(L, name).restype = C.c_int

    def timed(fn):
        t0 = time.perf_counter(); rc = fn(); return time.perf_counter() - t0, rc

    knobs = (C.c_int64 * 8)()
    L.ycge_debug_mesh_bvh_stats.restype, L.ycge_debug_mesh_bvh_stats.argtypes = abi.MESH_BVH_HOOK_PROTOTYPES["ycge_debug_mesh_bvh_stats"]
    L.ycge_debug_mesh_bvh_stats(None, knobs)          # (without a context: the knobs as the environment gives them - none set here - so [1] is the default of YCGE_MESH_BVH_DEVICE_MIN)
    L.ycge_debug_mesh_emit_stats.restype, L.ycge_debug_mesh_emit_stats.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_mesh_emit_stats"]
    emit_knobs = (C.c_int64 * 4)()
    L.ycge_debug_mesh_emit_stats(None, emit_knobs)
    default_min = max(int(knobs[1]), int(emit_knobs[1]))          # (... and of YCGE_MESH_EMIT_DEVICE_MIN: from here on an upload emits on the device)
    rows = []
    for label, tris in meshes:
        n = len(tris)
        t9 = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
        flat = flatten(scene_of(tris))
        nodes = np.zeros((2 * n, 10), np.float32); leaf = np.zeros(n, np.int32); st = np.zeros(3, np.int32); root = C.c_uint32(); tl = C.c_uint32()
        legs = {"host": [], "device": [], "device_emit": []}
        dev_build, host_build, arena, arena_tl, emit_build, emit_us, dev_records, dev_treelets = [], [], [], [], [], [], [], []
        res8 = np.zeros(abi.MESH_EMIT_RES_WORDS, np.uint32)
        for run in range(a.runs + 1):
            for leg, r in (("host", host_ctx), ("device", dev_ctx), ("device_emit", emit_ctx)):
                dt, rc = timed(lambda: L.ycge_scene_upload(r.ctx, flat.byref()))
                assert rc == 0, (label, leg, rc)
                if run:
                    legs[leg].append(dt)
            s = dev_ctx.mesh_bvh_stats()
            dt_b, _ = timed(lambda: L.ycge_host_build_mesh(C.c_void_p(t9.ctypes.data), n, C.c_void_p(nodes.ctypes.data), C.c_void_p(leaf.ctypes.data), C.c_void_p(st.ctypes.data)))
            dt_a, _ = timed(lambda: L.ycge_host_mesh_arena(C.c_void_p(t9.ctypes.data), n, None, C.c_int64(0), C.byref(root)))
            dt_t, _ = timed(lambda: L.ycge_host_mesh_arena_treelets(C.c_void_p(t9.ctypes.data), n, None, C.c_int64(0), C.byref(root), C.byref(tl)))
            rc = dev_arena(t9.ctypes.data, n, None, 0, C.byref(root), C.byref(tl), res8.ctypes.data)
            assert rc > 0, (label, rc)
            if run:
                dev_build.append(s["last_device_build_us"] * 1e-6); host_build.append(dt_b); arena.append(dt_a); arena_tl.append(dt_t)
                emit_build.append(emit_ctx.mesh_bvh_stats()["last_device_build_us"] * 1e-6); emit_us.append(emit_ctx.mesh_emit_stats()["last_device_emit_us"] * 1e-6)
                dev_records.append((int(res8[3]) + int(res8[4])) * 1e-6); dev_treelets.append(int(res8[5]) * 1e-6)
        es = emit_ctx.mesh_emit_stats()
        assert es["device_meshes"] == 1 and dev_ctx.mesh_emit_stats()["host_meshes"] == 1, (label, es)
        s = dev_ctx.mesh_bvh_stats()
        emit = max(0.0, med(arena) - med(host_build)); treelets = max(0.0, med(arena_tl) - med(arena))
        row = {"mesh": label, "triangles": n, "runs": a.runs, "host_build_ms": med(host_build), "device_build_ms": med(dev_build),
               "upload_host_ms": med(legs["host"]), "upload_device_ms": med(legs["device"]),
               "device_upload_split_ms": {"build": med(dev_build), "emit_mesh_records": emit, "append_treelets": treelets,
                                          "copies_and_rest": max(0.0, med(legs["device"]) - med(dev_build) - emit - treelets)},
               "upload_device_emit_ms": med(legs["device_emit"]),
               "device_emit_upload_split_ms": {"build": med(emit_build), "emit": med(dev_records), "treelets": med(dev_treelets),
                                               "copies_and_rest": max(0.0, med(legs["device_emit"]) - med(emit_build) - med(dev_records) - med(dev_treelets))},
               "device_emit_in_upload_ms": med(emit_us), "arena_bytes": es["arena_bytes"],
               "device_emit_no_slower": med(legs["device_emit"]) <= med(legs["device"]),
               "built_on_device": s["host_fallbacks"] == 0, "depth": s["max_depth"], "wide_nodes": s["wide_nodes"], "subtree_workgroups": s["subtree_workgroups"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    wins = [r["upload_device_emit_ms"] <= r["upload_host_ms"] for r in rows]          # (what an upload does from the crossover on: tree, records and treelets on the device)
    first = next((i for i in range(len(rows)) if all(wins[i:])), None)
    ok = [r["device_emit_no_slower"] for r in rows]
    first_ok = next((i for i in range(len(rows)) if all(ok[i:])), None)
    res = {"source_hash": build.source_hash(), "device": dev_ctx.device_name if hasattr(dev_ctx, "device_name") else "", "rows": rows,
           "crossover_triangles": rows[first]["triangles"] if first is not None else None, "device_wins_at_config_4": bool(wins[-1]),
           "device_emit_no_slower_from_default_min": all(r["device_emit_no_slower"] for r in rows if r["triangles"] >= default_min), "default_emit_device_min": default_min,
           "device_emit_crossover_triangles": rows[first_ok]["triangles"] if first_ok is not None else None}
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: res[k] for k in ("crossover_triangles", "device_wins_at_config_4", "device_emit_no_slower_from_default_min")}))
    host_ctx.close(); dev_ctx.close(); emit_ctx.close()


if __name__ == "__main__":
    main()
