"""Meshes attached to a resident scene (ycge_scene_attach_meshes) against the only other way to add one (ycge_scene_upload of the equivalent
scene), on the config-4 scene, one GPU - and what the re-homed arena does to a frame.

    python profiles/mesh_stream_rate.py --out DIR [--parent-lib PATH] [--rounds R] [--reps K] [--frames F]     -> DIR/mesh_stream_rate.json

Attach against upload.  A mesh of 1 000 / 16 000 / 131 072 drawn triangles joins config 4 (one mesh of 871 200 triangles).  Two legs,
alternated round by round in one process, the library calls alone on the clock (the records are made before):

    attach    ycge_scene_attach_meshes of the one mesh, then ycge_scene_update_objects with the object list that names it - on a context
              whose arena is pooled already; the objects are set back and the mesh detached off the clock.  The attach's own split - trees,
              emit, copies - comes from ycge_debug_mesh_pool_stats (host clock around each step, device waits included)
    upload    ycge_scene_upload of the equivalent scene (both meshes, the same objects) on a second context

The first attach's re-homing (the arena of config 4 moved into an allocation of twice its records, zeroed, two device copies) is timed on
a fresh context per round and reported on its own: the call, and its `copies` share.

The frame path.  A synchronous config-4 frame through this library before any attach, through this library after a re-homing attach that
was then detached (the arena has moved, nothing else has changed), and - with --parent-lib, a library built from the parent commit - through
that library on two contexts (what differs between two legs of ONE build is the noise the others are held against).  Legs alternated round
by round, each opening a round in turn; per leg median, min and p99 of a frame's wall time.

Each cell: median, min and p99 in microseconds.  Not measured: many small meshes per call, the C# wrapper, several GPUs.
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

SIZES = (1000, 16000, 131072)


def stats_us(t):
    t = np.asarray(t, np.float64) * 1e6
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "p99_us": float(np.percentile(t, 99)), "calls": int(t.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--frames", type=int, default=40)
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)

    from yetanotherconsolegameengine_amd import abi, build, scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten

    L = abi.load_library()
    sc, w, h, ss, pose = scenes.config_scene(4)
    flat = flatten(sc)
    n_prims = flat.struct.n_prims

    def context(lib=None):
        r = RaytraceRenderer(flat, w, h, pose.get("fov", 45.0), ss, lib=lib)
        r.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
        return r

    def drawn(n, seed):
        rng = np.random.default_rng(seed)
        c = np.asarray((1.6, 0.9, 1.0), np.float32) + rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
        return np.ascontiguousarray((c[:, None, :] + rng.uniform(-0.02, 0.02, (n, 3, 3)).astype(np.float32)).reshape(-1, 9), dtype=np.float32)

    def record(tris):
        m = abi.Mesh()
        m.triangles, m.n_triangles, m.material, m.tri_material = tris.ctypes.data_as(C.POINTER(C.c_float)), len(tris), 0, None
        return m

    def with_mesh(ref):
        """config 4's objects and one more: the mesh of index `ref`"""
        prims = (abi.Prim * (n_prims + 1))(*[flat.prims[i] for i in range(n_prims)])
        prims[n_prims].type, prims[n_prims].ref, prims[n_prims].material = abi.PRIM_MESH, ref, -1
        return prims

    base_prims = (abi.Prim * n_prims)(*[flat.prims[i] for i in range(n_prims)])
    n_up = flat.struct.n_meshes
    named = with_mesh(n_up)
    out1 = (C.c_int32 * 1)(-1)

    def stats(r):
        return r.mesh_pool_stats()

    # ---- the frame path, first, while the process has freed nothing yet: before any attach, after a re-homing attach that was detached, the
    # parent's library twice - the contexts made in the order parent A, this, parent B, this re-homed.  (In the committed run parent B ran
    # a fifth slower than parent A, the same library on the same scene, for all its rounds: unexplained - which is why the parent runs
    # twice and each of its legs is a yardstick of its own.)
    Lp = None
    if a.parent_lib:
        Lp = abi.bind(C.CDLL(str(a.parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if not n.startswith(("ycge_scene_attach_meshes", "ycge_scene_detach_meshes", "ycge_scene_append_materials",
                                                                                                                  "ycge_scene_attach_obj_mesh"))])          # (the parent has no such exports)
    parent_a = context(Lp) if Lp else None
    fresh = context()
    parent_b = context(Lp) if Lp else None
    moved = context()
    rec = (abi.Mesh * 1)(record(drawn(1000, 7)))
    moved._check(L.ycge_scene_attach_meshes(moved.ctx, rec, 1, out1))
    moved._check(L.ycge_scene_detach_meshes(moved.ctx, (C.c_int32 * 1)(out1[0]), 1))
    assert stats(moved)["pooled"] == 1 and stats(fresh)["pooled"] == 0
    legs = {"this, before any attach": fresh, "this, arena re-homed": moved}
    if Lp:
        legs["parent A"], legs["parent B"] = parent_a, parent_b
    periods = {k: [] for k in legs}
    order = list(legs)
    for rnd in range(a.rounds + 1):
        for k in order[rnd % len(order):] + order[:rnd % len(order)]:          # (the leg that opens a round pays for the pause before it: each leg opens in turn)
            r = legs[k]
            for _ in range(a.frames if rnd else 8):
                t0 = time.perf_counter()
                r.TryFlipAndBlit()
                dt = time.perf_counter() - t0
                if rnd:
                    periods[k].append(dt)
    frame_period = {k: stats_us(v) for k, v in periods.items()}
    same = all(np.array_equal(fresh.read(b), moved.read(b)) for b in (abi.BUF_CURRENT_HDR, abi.BUF_TAA_HISTORY))
    frame_period["re-homed frames equal the others bit for bit"] = bool(same)
    if a.parent_lib:
        # against each of the parent's legs on its own (pooled, a leg that runs apart from the other would widen the margin until it says nothing):
        # the leg's own min-to-p99 spread is the margin, the difference of the medians is what is held against it
        for leg in ("parent A", "parent B"):
            p = np.asarray(periods[leg]) * 1e6
            margin = float(np.percentile(p, 99) - p.min())
            cell = {"parent_median_us": float(np.median(p)), "parent_min_to_p99_us": margin}
            for k in ("this, before any attach", "this, arena re-homed"):
                d = float(np.median(periods[k]) * 1e6 - np.median(p))
                cell[k] = {"median_minus_parent_median_us": d, "within_the_parent_spread": bool(d <= margin)}
            frame_period["against " + leg] = cell
        frame_period["parent_legs_median_difference_us"] = float(abs(np.median(periods["parent A"]) - np.median(periods["parent B"])) * 1e6)
    for r in legs.values():
        r.close()

    # ---- attach against upload
    g, t = context(), context()
    warm = drawn(64, 1)
    g._check(L.ycge_scene_attach_meshes(g.ctx, (abi.Mesh * 1)(record(warm)), 1, out1))          # (the arena is pooled from here on; the warm mesh leaves again)
    g._check(L.ycge_scene_detach_meshes(g.ctx, (C.c_int32 * 1)(out1[0]), 1))
    res = {"what": "ycge_scene_attach_meshes + ycge_scene_update_objects against ycge_scene_upload of the equivalent scene on config 4, one MI355X; profiles/mesh_stream_rate.py",
           "scene": {"triangles": int(flat.n_triangles), "objects": int(n_prims), "frame": [w, h, ss]}, "frame_period": frame_period, "attach_against_upload": {}}
    for n in SIZES:
        tris = drawn(n, n)
        rec = (abi.Mesh * 1)(record(tris))
        eq = abi.Scene()
        C.memmove(C.byref(eq), C.byref(flat.struct), C.sizeof(eq))
        meshes = (abi.Mesh * (n_up + 1))(*[flat.meshes[i] for i in range(n_up)], rec[0])
        eq.meshes, eq.n_meshes, eq.prims, eq.n_prims = C.cast(meshes, C.POINTER(abi.Mesh)), n_up + 1, C.cast(named, C.POINTER(abi.Prim)), n_prims + 1
        times = {k: [] for k in ("attach", "update_objects", "attach+update_objects", "upload", "build", "emit", "copies")}
        builds = None
        for rnd in range(a.rounds + 1):          # round 0 warms both legs up and is dropped
            for _ in range(a.reps if rnd else 2):
                t0 = time.perf_counter()
                rc = L.ycge_scene_attach_meshes(g.ctx, rec, 1, out1)
                t1 = time.perf_counter()
                rc2 = L.ycge_scene_update_objects(g.ctx, named, n_prims + 1)
                t2 = time.perf_counter()
                g._check(rc); g._check(rc2)
                assert out1[0] == n_up
                st = stats(g)
                builds = (st["device_builds"], st["host_builds"])
                g._check(L.ycge_scene_update_objects(g.ctx, base_prims, n_prims))
                g._check(L.ycge_scene_detach_meshes(g.ctx, (C.c_int32 * 1)(n_up), 1))
                if rnd:
                    times["attach"].append(t1 - t0); times["update_objects"].append(t2 - t1); times["attach+update_objects"].append(t2 - t0)
                    times["build"].append(st["build_us"] * 1e-6); times["emit"].append(st["emit_us"] * 1e-6); times["copies"].append(st["copy_us"] * 1e-6)
            for _ in range(a.reps if rnd else 2):
                t0 = time.perf_counter()
                rc = L.ycge_scene_upload(t.ctx, C.byref(eq))
                dt = time.perf_counter() - t0
                t._check(rc)
                if rnd:
                    times["upload"].append(dt)
        cell = {k: stats_us(v) for k, v in times.items()}
        cell["upload_over_attach"] = cell["upload"]["median_us"] / cell["attach+update_objects"]["median_us"]
        cell["builds_since_the_upload"] = {"device": builds[0], "host": builds[1]}
        res["attach_against_upload"][str(n)] = cell
        t._check(L.ycge_scene_upload(t.ctx, flat.byref()))
    res["pool_after"] = stats(g)

    # ---- the first attach's re-homing, a fresh context per repetition
    first = {"attach": [], "copies": []}
    tris = drawn(1000, 7)
    rec = (abi.Mesh * 1)(record(tris))
    capacity = None
    for rnd in range(a.rounds + 1):
        r = context()
        t0 = time.perf_counter()
        rc = L.ycge_scene_attach_meshes(r.ctx, rec, 1, out1)
        dt = time.perf_counter() - t0
        r._check(rc)
        st = stats(r)
        assert st["pooled"] == 1 and st["growths"] == 0
        capacity = st["capacity_units"]
        if rnd:
            first["attach"].append(dt); first["copies"].append(st["copy_us"] * 1e-6)
        r.close()
    res["first_attach_rehoming"] = {"mesh_triangles": 1000, "capacity_units": capacity, "arena_bytes": capacity * (32 + 256), "attach": stats_us(first["attach"]),
                                    "copies": stats_us(first["copies"])}

    res["source_hash"] = build.source_hash()
    res["device"] = str(g.device_info())
    (out / "mesh_stream_rate.json").write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
