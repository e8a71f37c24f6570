"""Chunk generation rates (ycge_scene_generate_grids) on the 17 x 17 x 8 view of BuildMinecraftLike's config - chunk 32, 32 x 8 x 32 chunks,
seed 0, world_min (-512, 0, -512) - around the default camera:

  * one ycge_scene_generate_grids call for the whole view (2 312 keys), and one border crossing (17 x 8 keys);
  * the same two done the only way a build without the export can: ycge_worldgen_chunk_cells per key on the host, then ycge_scene_attach_grids.

Medians over repeated runs (a fresh context each: an attach into a warm arena is another measurement), written to
profiles/worldgen_rate.json.  The host generator runs over the FULL key list, one thread, --host-runs times (it is deterministic CPU
work of minutes for the view: the default is one run, and the JSON says how many).

    python profiles/worldgen_rate.py [--runs 5] [--host-runs 1]
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
from yetanotherconsolegameengine_amd import abi, build, scenes, world_file          # noqa: E402
from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer    # noqa: E402
from yetanotherconsolegameengine_amd.scene import AmbientLight, Material, Scene, Sphere, ZERO, flatten, vec3          # noqa: E402

S, CHUNKS_Y, VIEW = 32, 8, 8


def anchor():
    s = Scene()
    s.IsVolumeScene = True
    s.Ambient = AmbientLight(vec3(1, 1, 1), 0.0)
    lights, top, bottom = scenes.sun_moon_lights(0.4)
    s.Lights.extend(lights)
    s.BackgroundTop, s.BackgroundBottom = top, bottom
    for k in range(27):
        s.Add(Sphere(vec3(0, -500, 0), 0.1, Material(vec3(0.1 + 0.03 * k, 0.5, 0.9 - 0.03 * k), 0.1, 0.0, ZERO)))
    return flatten(s)


def proto():
    pairs = [(m, k) for m in range(1, 9) for k in range(3)]
    lk = (abi.VoxelLookup * len(pairs))(*[abi.VoxelLookup(a, b, (a * 3 + b) % 27) for a, b in pairs])
    g = abi.Grid()
    g.lookup, g.n_lookup, g.default_material = C.cast(lk, C.POINTER(abi.VoxelLookup)), len(pairs), -1
    g.wireframe, g.wire_width_fraction, g.wire_max_distance = 1, 0.06, 16.0
    g.voxel_size = abi.Vec3(1, 1, 1)
    return g, lk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=1)
    a = ap.parse_args()
    world = abi.World(S, CHUNKS_Y, 0, abi.Vec3(-512, 0, -512), abi.Vec3(1, 1, 1))
    camera, wmin, vox = (0.0, 120.0, 0.0), (-512.0, 0.0, -512.0), (1.0, 1.0, 1.0)          # scene.DefaultCameraPos, VolumeScenes.cs:594
    view = world_file.build_desired_set(camera, wmin, vox, S, VIEW, CHUNKS_Y)
    cx0, cz0 = world_file.center_column(camera, wmin, vox, S)
    border = [(cx0 + VIEW + 1, cy, cz) for cz in range(cz0 - VIEW, cz0 + VIEW + 1) for cy in range(CHUNKS_Y)]          # what enters when the camera crosses into column cx0 + 1
    g, keep = proto()
    L = abi.load_library()
    out = {"build": build.source_hash(), "chunk": S, "view_keys": len(view), "border_keys": len(border), "runs": a.runs}
    for name, keys in (("view", view), ("border", border)):
        gen_s, kern = [], []
        for _ in range(a.runs):
            r = RaytraceRenderer(anchor(), 96, 27)
            t0 = time.perf_counter()
            idx = r.GenerateGrids(world, keys, g)
            gen_s.append(time.perf_counter() - t0)
            kern.append(r.worldgen_stats())
            r.close()
        out[name] = {"generate_grids_ms_median": 1e3 * statistics.median(gen_s), "generate_grids_ms_all": [1e3 * v for v in gen_s],
                     "columns_kernel_us_median": statistics.median(k["last_columns_us"] for k in kern),
                     "fill_tree_kernels_us_median": statistics.median(k["last_fill_us"] for k in kern), "resident": sum(i >= 0 for i in idx)}
        # the parent commit's way: the host generator for every key, then ycge_scene_attach_grids with the cells of the chunks that hold something
        cells = np.zeros((len(keys), S, S, S, 2), np.int32)
        any_ = (C.c_int32 * len(keys))()
        host_s = []
        for _ in range(a.host_runs):
            t0 = time.perf_counter()
            for j, k in enumerate(keys):
                L.ycge_worldgen_chunk_cells(C.byref(world), *k, cells[j].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(any_, 4 * j))
            host_s.append(time.perf_counter() - t0)
        solid = [j for j in range(len(keys)) if any_[j]]
        att = []
        for _ in range(a.runs):
            r = RaytraceRenderer(anchor(), 96, 27)
            recs = (abi.Grid * len(solid))()
            for n, j in enumerate(solid):
                C.memmove(C.byref(recs[n]), C.byref(g), C.sizeof(abi.Grid))
                recs[n].nx = recs[n].ny = recs[n].nz = S
                recs[n].min_corner = abi.Vec3(*[wmin[ax] + keys[j][ax] * S for ax in range(3)])
                recs[n].cells = cells[j].ctypes.data_as(C.POINTER(C.c_int32))
            o = (C.c_int32 * len(solid))()
            t0 = time.perf_counter()
            r._check(L.ycge_scene_attach_grids(r.ctx, recs, len(solid), o))
            att.append(time.perf_counter() - t0)
            r.close()
        assert len(solid) == out[name]["resident"]
        out[name]["host_generator_ms_median"] = 1e3 * statistics.median(host_s)
        out[name]["host_generator_runs"] = a.host_runs
        out[name]["attach_ms_median"] = 1e3 * statistics.median(att)
        out[name]["host_then_attach_ms"] = 1e3 * (statistics.median(host_s) + statistics.median(att))
        del cells
    (ROOT / "profiles" / "worldgen_rate.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
