"""MeshScenes.AddMeshAutoGround's tail on a held OBJ (ycge_obj_ground): the kernels of csrc/ycge_obj_ground.hip against what they replace,
ycge_obj_read followed by ycge_obj_ground_host on the same arrays.  Both sides are C++ and both are timed in this process.  One GPU.
Recorded, nothing gated.

    python profiles/obj_ground_rate.py [--out profiles/obj_ground_rate.json] [--runs 5]

Meshes, drawn from a seed: scenes.make_torus_knot at 1 000, 16 000, 131 072 and 871 200 triangles (the last is config 4's size) with three
islands of three faces each, written as OBJ text with %.9g and parsed by ycge_obj_parse.  For each:
  device   ycge_obj_ground on the held OBJ with YCGE_OBJ_GROUND_DEVICE_MIN = 0: the median of --runs calls after one warm-up, min and max
           beside it; the labelling rounds (ycge_debug_obj_ground_stats)
  host     ycge_obj_read into page-locked arrays followed by ycge_obj_ground_host on them, the same way
  phases   a second context made with YCGE_OBJ_GROUND_PHASES (a stream synchronise behind every phase, so their sum is above the plain
           call): labelling, count + winner, terms, the three serial sums, bounds + read-back, each the median of --runs
           (ycge_debug_obj_ground_phases) - whether the serial sums dominate
`crossover_triangles` is the smallest measured size from which the device tail is no slower than the host side at every larger measured
size (null: the host side was faster at the largest size); `device_min_default` is the value YCGE_OBJ_GROUND_DEVICE_MIN_DEFAULT
(csrc/ycge_ctx.h) is set from: the crossover, or INT32_MAX when there is none, so that the host tail runs."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np

SIZES = {1000: (25, 20), 16000: (100, 80), 131072: (256, 256), 871200: (1320, 330)}          # make_torus_knot(u, v): 2 u v triangles


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def obj_text(pos, faces) -> bytes:
    v = "\n".join("v %.9g %.9g %.9g" % (x, y, z) for x, y, z in pos.tolist())
    f = "\n".join("f %d %d %d" % (a + 1, b + 1, c + 1) for a, b, c in faces.tolist())
    return (v + "\n" + f + "\n").encode()


def mesh(rng, u, v):
    from yetanotherconsolegameengine_amd import scenes
    pos, faces = scenes.make_torus_knot(u, v)
    pos, faces = np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    base = len(pos)
    isl_pos = rng.uniform(5.0, 9.0, size=(15, 3)).astype(np.float32)
    isl = [np.array([[base + 5 * k + i, base + 5 * k + i + 1, base + 5 * k + i + 2] for i in range(3)], np.int32) for k in range(3)]
    half = len(faces) // 2
    return np.vstack([pos, isl_pos]), np.vstack([isl[0], faces[:half], isl[1], faces[half:], isl[2]])


def timed_ms(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def context(**env):
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    env = {"YCGE_OBJ_GROUND_DEVICE_MIN": "0", **env}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return RaytraceRenderer(None, 64, 36)          # (the knobs are read once, at ycge_create)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "obj_ground_rate.json"))
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("profiles/obj_ground_rate.py measures on the GPU: none found (nothing is written)")
    torch.zeros(1, device="cuda")
    from yetanotherconsolegameengine_amd import abi
    r, rp = context(), context(YCGE_OBJ_GROUND_PHASES="1")
    L = r.L
    for name in ("ycge_obj_ground_host", "ycge_obj_ground", "ycge_obj_read"):
        getattr(L, name).restype, getattr(L, name).argtypes = abi._PROTOTYPES[name]
    rng = np.random.default_rng(20261)
    result = {"device": r.device_info()[0], "runs": a.runs, "unit": "ms", "sizes": []}
    for want, (u, v) in SIZES.items():
        pos, faces = mesh(rng, u, v)
        data = obj_text(pos, faces)
        info = r.ParseObj(data)
        rp.ParseObj(data)
        ground, host_ground = abi.ObjGroundInfo(), abi.ObjGroundInfo()
        hpos, h1 = r._page_locked_zeros((info.n_positions, 3), np.float32)
        hfaces, h2 = r._page_locked_zeros((info.n_triangles, 3), np.int32)

        def device():
            r._check(L.ycge_obj_ground(r.ctx, C.byref(ground)))

        def host():
            r._check(L.ycge_obj_read(r.ctx, hpos.ctypes.data, hfaces.ctypes.data))
            assert L.ycge_obj_ground_host(hpos.ctypes.data, info.n_positions, hfaces.ctypes.data, info.n_triangles, C.byref(host_ground)) == 0

        def host_tail_alone():
            L.ycge_obj_ground_host(hpos.ctypes.data, info.n_positions, hfaces.ctypes.data, info.n_triangles, C.byref(host_ground))

        dev = stats(timed_ms(device, a.runs))
        st = r.obj_ground_stats()
        hst = stats(timed_ms(host, a.runs))
        alone = stats(timed_ms(host_tail_alone, a.runs))
        assert ground.on_device == 1 and bytes(ground)[:56] == bytes(host_ground)[:56], "the two sides disagree"
        phases = {k[:-3]: [] for k in abi.OBJ_GROUND_PHASES}          # label, select, terms, sums, bounds: ms like everything else here
        for it in range(a.runs + 1):
            rp.ObjGround()
            if it:
                st_p = rp.obj_ground_stats()
                for k in phases:
                    phases[k].append(st_p[k + "_us"] / 1e3)
        row = {"triangles": info.n_triangles, "positions": info.n_positions, "parsed_on_device": int(info.on_device), "rounds": st["rounds"],
               "device_ycge_obj_ground": dev, "host_read_plus_ground_host": hst, "host_ground_host_alone": alone,
               "device_phases": {k: stats(v) for k, v in phases.items()}}
        result["sizes"].append(row)
        print(want, json.dumps(row), flush=True)
    cross = None
    for row in reversed(result["sizes"]):
        if row["device_ycge_obj_ground"]["median"] <= row["host_read_plus_ground_host"]["median"]:
            cross = row["triangles"]
        else:
            break
    result["crossover_triangles"] = cross
    result["device_min_default"] = cross if cross is not None else 2147483647
    result["crossover_note"] = ("smallest measured size from which ycge_obj_ground on the device is no slower than ycge_obj_read + ycge_obj_ground_host at every larger "
                                "measured size (null: the host side was faster at the largest size, and the default sends every OBJ to the host tail)")
    r.close(); rp.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
