"""The adaptive sixel palette on the device: call time and stream bytes of `_sixel_palette` (hold 0 and hold 1) against `_sixel` plain and
dithered, for traced frames (at rest and with the camera moving) and for video; the picture's error against the RGBA plane for the three
forms; the histogram on a flat against a noisy plane; and what the existing calls cost against the parent commit's library.  One GPU, one
process, one run.

    python profiles/sixel_palette_rate.py [--parent-lib PATH --rounds 6 --frames-per-round 8]     -> profiles/sixel_palette_rate.json

The geometry of profiles/sixel_rate.json: config 4 in a 240 x 67 framebuffer at super_sample 8 - 1920 x 1072 pixels; the video source is the
1920 x 1080 BGR frame of profiles/sixel_delta_rate.py.  Streams go into a pageable array of the bound's size.  The host clock around the
calls, variants on contexts of their own, alternated round by round (profiles/sixel_rate.py's `timed`); per variant the median, minimum and
99th percentile of the rounds.  With --parent-lib: `_sixel`, `_ansi_rgb_delta` and plain ycge_render_frame through this library against the
parent commit's, two parent contexts and one product context alternated; unmoved means within the spread the parent's two contexts show.
The kernels' own times come from a kernel trace of `--trace-frames N` (this script run under the profiler; merged under "kernel_us" by
--merge-trace FILE, a kernel-stats CSV).  Nothing here measures the terminal that consumes the bytes, nor the C# wrappers.
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

import sixel_delta_rate as DR
import sixel_rate as R

U8P = C.POINTER(C.c_uint8)
W, H, SS = R.W, R.H, R.SS
PW, PH = W * SS, 2 * H * SS
SRC_W, SRC_H, BPP = DR.SRC_W, DR.SRC_H, DR.BPP
NEW_EXPORTS = ("ycge_sixel_palette_stream_bound", "ycge_render_frame_sixel_palette", "ycge_video_blit_sixel_palette", "ycge_render_frame_pixels_palette",
               "ycge_video_blit_pixels_palette", "ycge_sixel_palette_host", "ycge_sixel_encode_palette_host")


def fns_of(g):
    """name -> callable rendering one frame (or blitting one source) as a stream and returning its length"""
    cap = g.sixel_palette_stream_bound(PW, PH, g.L)
    out, n = np.empty(cap, np.uint8), C.c_size_t(0)
    p = out.ctypes.data_as(U8P)

    def cube(dither=0):
        g._check(g.L.ycge_render_frame_sixel(g.ctx, 0, 0, 0, dither, p, cap, C.byref(n), None, None))
        return n.value

    def adaptive(hold=0):
        g._check(g.L.ycge_render_frame_sixel_palette(g.ctx, 0, 0, 0, hold, p, cap, C.byref(n), None, None, None, None))
        return n.value

    def video_cube(frame, dither=0):
        g._check(g.L.ycge_video_blit_sixel(g.ctx, frame.ctypes.data_as(U8P), SRC_W, SRC_H, BPP, 0, 0, 0, dither, p, cap, C.byref(n), None))
        return n.value

    def video_adaptive(frame, hold=0):
        g._check(g.L.ycge_video_blit_sixel_palette(g.ctx, frame.ctypes.data_as(U8P), SRC_W, SRC_H, BPP, 0, 0, 0, hold, p, cap, C.byref(n), None, None, None))
        return n.value
    return {"cube": cube, "adaptive": adaptive, "video cube": video_cube, "video adaptive": video_adaptive, "_keep": out}


FORMS = {"sixel": ("cube", 0), "sixel dither": ("cube", 1), "palette hold 0": ("adaptive", 0), "palette hold 1": ("adaptive", 1)}


def sizes(v):
    return {"mean": float(np.mean(v)), "min": int(np.min(v)), "max": int(np.max(v))}


def frames_section(rounds, frames, settle):
    ctxs = {k: R.renderer() for k in FORMS}
    f = {k: fns_of(g) for k, g in ctxs.items()}
    fns = {k: (lambda k=k: f[k][FORMS[k][0]](FORMS[k][1])) for k in FORMS}
    for fn in fns.values():
        for _ in range(settle):
            fn()
    per, _ = R.timed(fns, rounds, frames)
    rest = {k: [fn() for _ in range(frames)] for k, fn in fns.items()}
    moving = {k: [] for k in fns}
    for j in range(frames):
        for k, g in ctxs.items():
            R.move(g, j + 1)
            moving[k].append(fns[k]())
    for g in ctxs.values():
        g.close()
    res = {"ms_per_frame_at_rest": {k: R.stats(v) for k, v in per.items()}, "bytes_at_rest": {k: sizes(v) for k, v in rest.items()},
           "bytes_moving": {k: sizes(v) for k, v in moving.items()}, "rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle,
           "note": "hold 1 with the camera moving maps every frame through the palette of the resting picture"}
    print("frames", json.dumps(res), flush=True)
    return res


def video_section(rounds, frames):
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    still = DR.source(0)
    changing = [DR.source(k) for k in range(1, 5)]
    video = {"sixel": ("video cube", 0), "sixel dither": ("video cube", 1), "palette hold 0": ("video adaptive", 0), "palette hold 1": ("video adaptive", 1)}
    ctxs = {k: RaytraceRenderer(None, W, H, 45.0, SS) for k in video}
    f = {k: fns_of(g) for k, g in ctxs.items()}
    turn = {"n": 0}

    def nxt():
        turn["n"] += 1
        return changing[turn["n"] % len(changing)]
    fns = {k: (lambda k=k: f[k][video[k][0]](still, video[k][1])) for k in video}
    moving = {k: (lambda k=k: f[k][video[k][0]](nxt(), video[k][1])) for k in video}
    for fn in fns.values():
        fn(); fn()
    per, _ = R.timed(fns, rounds, frames)
    still_bytes = {k: [fn() for _ in range(4)] for k, fn in fns.items()}
    per_moving, _ = R.timed(moving, rounds, frames)
    moving_bytes = {k: [fn() for _ in range(8)] for k, fn in moving.items()}
    for g in ctxs.values():
        g.close()
    res = {"ms_per_call_still": {k: R.stats(v) for k, v in per.items()}, "ms_per_call_changing": {k: R.stats(v) for k, v in per_moving.items()},
           "bytes_still": {k: sizes(v) for k, v in still_bytes.items()}, "bytes_changing": {k: sizes(v) for k, v in moving_bytes.items()}}
    print("video", json.dumps(res), flush=True)
    return res


def quality(settle):
    """RMS error of the bytes a terminal shows (percentages back to bytes, p * 255 / 100) against the RGBA plane, one resting frame"""
    import sixel_restatement as X
    g = R.renderer()
    for _ in range(settle):
        g.TryFlipAndBlit(want_sdr=True)
    planes = g.TryFlipAndBlitPixelsPalette()
    rgb = planes["rgba"][..., :3].astype(np.int64)
    res = {"registers": planes["count"]}
    pct = (200 * planes["palette"][:, :3].astype(np.int64) + 255) // 510
    rms = lambda shown: float(np.sqrt(((shown - rgb) ** 2).mean()))
    res["adaptive"] = rms((pct * 255 // 100)[planes["index"]])
    res["adaptive_register_bytes"] = rms(planes["palette"][:, :3].astype(np.int64)[planes["index"]])
    for name, dither in (("cube", 0), ("cube dithered", 1)):
        index = X.quantise(rgb, dither).astype(np.int64)
        res[name] = rms(np.stack([index // 36, index // 6 % 6, index % 6], axis=-1) * 20 * 255 // 100)
    res["note"] = "the cube figures quantise the same RGBA plane by the contract's integer rule (tests/sixel_restatement.quantise)"
    g.close()
    print("quality", json.dumps(res), flush=True)
    return res


def histogram_planes(reps=20):
    """the palette stage alone through its hook on a flat and on a noisy 1920 x 1072 plane: host clock around the call, which also uploads
    the plane and reads the palette back - the kernels' own times are the trace's"""
    from yetanotherconsolegameengine_amd import abi
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    g = RaytraceRenderer(None, 16, 8, 45.0, 1)
    fn = g.L.ycge_test_sixel_palette
    fn.restype, fn.argtypes = abi.SIXEL_PALETTE_HOOK_PROTOTYPES["ycge_test_sixel_palette"]
    rng = np.random.default_rng(3)
    planes = {"flat": np.full((PH, PW, 4), (97, 160, 229, 255), np.uint8), "noisy": np.concatenate([rng.integers(0, 256, (PH, PW, 3), np.uint8), np.full((PH, PW, 1), 255, np.uint8)], axis=2)}
    res = {}
    count = C.c_int32(0)
    for name, p in planes.items():
        p = np.ascontiguousarray(p)
        times = []
        for hold in (0, 1):
            for _ in range(reps):
                t0 = time.perf_counter()
                g._check(fn(g.ctx, p.ctypes.data_as(U8P), PW, PH, hold, None, None, None, C.byref(count)))
                times.append((time.perf_counter() - t0) * 1e3)
            res[name + (" hold 1 (no build)" if hold else " hold 0 (build)")] = R.stats(times[-reps + 2:])
        res[name + " registers"] = count.value
    res["build_ms_by_difference"] = {k: res[k + " hold 0 (build)"]["median"] - res[k + " hold 1 (no build)"]["median"] for k in planes}
    g.close()
    print("histogram", json.dumps(res), flush=True)
    return res


def against_parent(parent_lib, rounds, frames, settle):
    from yetanotherconsolegameengine_amd import abi
    P = abi.bind(C.CDLL(str(parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n not in NEW_EXPORTS])
    assert not hasattr(P, NEW_EXPORTS[0]), "the parent's library is expected to lack the new exports"
    ctxs = {"parent A": R.renderer(P), "product": R.renderer(), "parent B": R.renderer(P)}
    fns = {k: R.frame_fns(g, sixel=True) for k, g in ctxs.items()}
    res = {"rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle, "calls": {}}
    for call in ("sixel", "ansi rgb delta", "render_frame"):
        for f in fns.values():
            for _ in range(settle):
                f[call]()
        per, _ = R.timed({k: f[call] for k, f in fns.items()}, rounds, frames)
        parent = per["parent A"] + per["parent B"]
        spread = float(np.max(parent) - np.min(parent))
        diff = float(np.median(per["product"]) - np.median(parent))
        res["calls"][call] = {"ms_per_frame": {k: R.stats(v) for k, v in per.items()}, "parent_median_ms": float(np.median(parent)), "parent_spread_ms": spread,
                              "product_minus_parent_ms": diff, "not_slower_by_more_than_the_parents_spread": bool(diff <= spread)}
        print("parent:", call, json.dumps(res["calls"][call]), flush=True)
    for g in ctxs.values():
        g.close()
    return res


def trace_frames(n):
    """n frames of each new form, then the stage alone on a flat and a noisy plane (histogram_planes), for a kernel trace taken from outside"""
    g = R.renderer()
    f = fns_of(g)
    for hold in (0, 1):
        for k in range(n):
            f["adaptive"](hold)
    src = DR.source(0)
    for k in range(n):
        f["video adaptive"](src, 0)
    g.close()
    histogram_planes(reps=4)


def merge_trace(stats_csv, out):
    """kernel_us from a kernel-stats CSV (columns Name, Calls, AverageNs, MinNs, MaxNs as the profiler writes them)"""
    m = json.loads(Path(out).read_text())
    rows = {}
    with open(stats_csv, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            if "k_pal_" in name or "k_sixel_" in name or "k_video_pixels" in name:
                short = name.split("(")[0].replace("(anonymous namespace)::", "").replace("void ", "")
                rows[short] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    m["kernel_us"] = rows
    Path(out).write_text(json.dumps(m, indent=1) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames-per-round", type=int, default=8)
    ap.add_argument("--settle", type=int, default=40)
    ap.add_argument("--trace-frames", type=int, default=0)
    ap.add_argument("--merge-trace", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sixel_palette_rate.json"))
    a = ap.parse_args()
    if a.trace_frames:
        trace_frames(a.trace_frames)
        sys.exit(0)
    if a.merge_trace:
        merge_trace(a.merge_trace, a.out)
        sys.exit(0)
    m = {"what": "the adaptive sixel palette on one MI355X; profiles/sixel_palette_rate.py", "config": R.CONFIG, "framebuffer": [W, H],
         "super_sample": SS, "pixels": [PW, PH], "video_source": [SRC_W, SRC_H, BPP], "kernel_us": "not yet run",
         "not_measured": "the terminal that consumes the bytes, and the C# wrappers (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    m["frames"] = frames_section(a.rounds, a.frames_per_round, a.settle)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
    m["video"] = video_section(a.rounds, a.frames_per_round)
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
    m["quality_rms_error_of_a_resting_frame"] = quality(a.settle)
    m["palette_stage_on_a_flat_and_a_noisy_plane"] = histogram_planes()
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
    m["existing_calls_against_parent"] = against_parent(a.parent_lib, a.rounds, a.frames_per_round, a.settle) if a.parent_lib else "not measured"
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
