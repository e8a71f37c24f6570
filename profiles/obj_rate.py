"""OBJ meshes from file bytes (ycge_obj_parse / ycge_obj_triangles): what reading a mesh file costs on the host's one thread, in the
library's host parser and on the device.  One GPU, one process.  Recorded, nothing gated.

    python profiles/obj_rate.py [--out profiles/obj_rate.json] [--runs 5] [--loader-runs 3]

Files, written to a temporary directory from a seed: config 4's stand-in mesh (scenes.make_torus_knot, 871 200 triangles) as OBJ text
with %.6f coordinates and once with %.9g, and the bunny asset with %.6f.  For each file:
  (a) loader    mesh_loader.load_obj(path) - the per-line interpreter loop a Python user has today (median of --loader-runs after one
                warm-up: it takes seconds a run and does not touch the GPU)
  (b) host      ycge_obj_parse_host, counts and arrays (one call with both arrays given)
  (c) device    ycge_obj_parse + ycge_obj_triangles from page-locked text, the host clock around each call (both return synchronised),
                split by ycge_debug_obj_stats into: upload (the parse call minus its two kernel phases: staging, copy, allocations),
                lines (marking, line walk, scans, two read-backs of counts), parse (token parsing, used / range / bounds), triangles
                (the gather kernel and its bounds), read-back (the triangles call minus its kernel phase: 36 bytes a triangle to the host)
Each is the median of --runs after one warm-up, with min and max beside it.  A file the kernels decline (on_device = 0, last_decline: why)
is read by the host parser inside ycge_obj_parse: its parse_call is then the host parser's time plus the upload of the arrays.
The crossover: prefixes of the %.6f stand-in file cut at a face boundary (about 1 KB .. 4 MB), (b) against (c)'s parse call alone;
`crossover_bytes` is the smallest measured size from which the device parse is no slower at every larger measured size - the figure
YCGE_OBJ_DEVICE_MIN's default is set from (csrc/ycge_ctx.h)."""
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


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def obj_text(pos, faces, fmt) -> bytes:
    v = "\n".join(("v " + fmt + " " + fmt + " " + fmt) % (x, y, z) for x, y, z in pos.tolist())
    f = "\n".join("f %d %d %d" % (a + 1, b + 1, c + 1) for a, b, c in faces.tolist())
    return (v + "\n" + f + "\n").encode()


def timed(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure_device(r, data, runs):
    """ms per run of each part of (c) on page-locked text"""
    from yetanotherconsolegameengine_amd import abi
    L, n = r.L, len(data)
    p = C.c_void_p()
    r._check(L.ycge_alloc_host_buffer(n, C.byref(p)))
    C.memmove(p, data, n)
    info = abi.ObjInfo()
    rows = {k: [] for k in ("parse_call", "triangles_call", "upload", "lines", "parse", "triangles", "read_back", "total")}
    try:
        tris = None
        for it in range(runs + 1):
            t0 = time.perf_counter()
            r._check(L.ycge_obj_parse(r.ctx, p, n, C.byref(info)))
            t1 = time.perf_counter()
            if tris is None:
                tris, h = r._page_locked_zeros((info.n_triangles, 3, 3), np.float32)
                bounds = np.zeros(6, np.float32)
                t1 = time.perf_counter()
            t = (C.c_float * 3)(0.25, 0.5, -1.0)
            r._check(L.ycge_obj_triangles(r.ctx, 1, 1.0, 1.5, t, tris.ctypes.data, bounds.ctypes.data))
            t2 = time.perf_counter()
            st = r.obj_stats()
            if it == 0:
                continue
            pc, tc = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            rows["parse_call"].append(pc); rows["triangles_call"].append(tc); rows["total"].append(pc + tc)
            rows["lines"].append(st["lines_us"] / 1e3); rows["parse"].append(st["parse_us"] / 1e3); rows["triangles"].append(st["triangles_us"] / 1e3)
            rows["upload"].append(pc - (st["lines_us"] + st["parse_us"]) / 1e3); rows["read_back"].append(tc - st["triangles_us"] / 1e3)
    finally:
        L.ycge_obj_release(r.ctx)
        L.ycge_free_host_buffer(p)
    out = {k: stats(v) for k, v in rows.items()}
    out["on_device"], out["last_decline"] = int(info.on_device), st["last_decline"]          # (declined: the host parser's time is in parse_call, the split says nothing)
    return out, (info.n_positions, info.n_triangles, int(info.n_lines))


def measure_host(L, data, runs):
    from yetanotherconsolegameengine_amd import abi
    pos, faces, info = abi.obj_parse_host(data, L)
    fn = L.ycge_obj_parse_host
    return stats(timed(lambda: fn(data, len(data), pos.ctypes.data, faces.ctypes.data, C.byref(info), None, 0), runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "obj_rate.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--loader-runs", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a rehearsal: a small stand-in mesh")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("profiles/obj_rate.py measures on the GPU: none found (nothing is written)")
    torch.zeros(1, device="cuda")
    from yetanotherconsolegameengine_amd import abi, mesh_loader, scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    r = RaytraceRenderer(None, 64, 36)
    knot = scenes.make_torus_knot(*((64, 16) if a.small else (1320, 330)))
    bunny = scenes.load_bunny_arrays()
    files = {"stand_in_%.6f": obj_text(*knot, "%.6f"), "stand_in_%.9g": obj_text(*knot, "%.9g"), "bunny_%.6f": obj_text(*bunny, "%.6f")}
    result = {"device": r.device_info()[0], "runs": a.runs, "loader_runs": a.loader_runs, "unit": "ms", "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, data in files.items():
            path = Path(tmp) / "mesh.obj"
            path.write_bytes(data)
            dev, counts = measure_device(r, data, a.runs)
            row = {"bytes": len(data), "positions": counts[0], "triangles": counts[1], "lines": counts[2],
                   "a_mesh_loader_load_obj": stats(timed(lambda: mesh_loader.load_obj(path), a.loader_runs)),
                   "b_ycge_obj_parse_host": measure_host(r.L, data, a.runs), "c_device": dev}
            result["files"][name] = row
            print(name, json.dumps(row), flush=True)
    # the crossover between (b) and the parse call of (c): prefixes of the first file, cut behind a whole face line
    base = files["stand_in_%.6f"]
    head_end = base.index(b"\nf ") + 1
    sweep = []
    for want in (1 << 10, 4 << 10, 16 << 10, 64 << 10, 256 << 10, 1 << 20, 4 << 20):
        nv = max(3, want // 60)          # about half the bytes in positions
        vs = base[:head_end].split(b"\n")[:nv]
        fs = [b"f %d %d %d" % (k % nv + 1, (k + 1) % nv + 1, (k + 2) % nv + 1) for k in range(max(1, want // 40))]
        data = b"\n".join(vs + fs) + b"\n"
        dev, _ = measure_device(r, data, a.runs)
        host = measure_host(r.L, data, a.runs)
        sweep.append({"bytes": len(data), "host": host, "device_parse_call": dev["parse_call"]})
        print("sweep", json.dumps(sweep[-1]), flush=True)
    cross = None
    for k in range(len(sweep) - 1, -1, -1):
        if sweep[k]["device_parse_call"]["median"] <= sweep[k]["host"]["median"]:
            cross = sweep[k]["bytes"]
        else:
            break
    result["sweep"] = sweep
    result["crossover_bytes"] = cross
    result["crossover_note"] = "smallest measured size from which ycge_obj_parse on the device is no slower than ycge_obj_parse_host at every larger measured size (null: the host parser was faster at the largest size)"
    r.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
