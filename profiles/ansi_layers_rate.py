"""The layered ANSI streams on the device (ycge_console_set_layers): what a synchronous frame of `_ansi`, `_ansi_delta` and `_ansi_rgb_delta`
costs with the reference's arrangement of framebuffers against the same call with none, and what the unlayered calls cost against the
parent commit's library.  One GPU, one process, one run.

    python profiles/ansi_layers_rate.py [--parent-lib PATH --rounds 8 --frames-per-round 10]     -> profiles/ansi_layers_rate.json

Config 4 at 1920 x 540 under a 1921 x 541 console, the camera at rest, every context converged before anything is timed, every stream into
page-locked memory of the library, the host clock around the calls, variants alternated round by round (the order reversed on odd rounds),
per variant the median, minimum and maximum of the rounds.

(a) Layered against unlayered.  The layers: a console-sized bottom framebuffer below the raytrace one, blank but for one text row, and a
40 x 10 framebuffer above.  Three variants per call on contexts of their own: `none`, `layers` (set once, the stream calls alone are timed)
and `layers+set` (the text row changes every frame: one ycge_console_set_layers call in front of every stream call, timed with it - the
29 MB of console-sized cells go up each time).  Reported: frame ms, bytes a frame, and the difference against the spread (max - min) of the
`none` variant's rounds.
(b) Unlayered against the parent.  With --parent-lib, the parent commit's library, built elsewhere from the parent's sources, is loaded
beside the product's: two parent contexts and one product context run the three calls with no layers, alternated.  The parent's own
spread is max - min over the rounds of both its contexts; the product agrees when its median lies within that spread of the median of the
parent's rounds.  Without --parent-lib this part is "not measured".
Nothing here measures the terminal that consumes the bytes, nor the host that fills the framebuffers.
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

U8P = C.POINTER(C.c_uint8)
CALLS = ("ansi", "ansi delta", "ansi rgb delta")
GAP, TOL = 3, 0


def renderer(lib=None):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(4)
    g = RaytraceRenderer(flatten(sc), w, h, pose.get("fov", 45.0), ss, lib=lib)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    return g


def frame_fns(g):
    """call name -> a callable rendering one frame into page-locked memory and returning the stream's length"""
    cw, ch = g.fbW + 1, g.fbH + 1
    cap = g.ansi_rgb_stream_bound(cw, ch, g.L)
    out = g._page_locked_zeros((cap,), np.uint8)[0]
    p, n, info = out.ctypes.data_as(U8P), C.c_size_t(0), (C.c_uint32 * 4)()

    def stream():
        g._check(g.L.ycge_render_frame_ansi(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
        return n.value

    def delta():
        g._check(g.L.ycge_render_frame_ansi_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, GAP, 0, p, cap, C.byref(n), info, None, None))
        return n.value

    def rgb_delta():
        g._check(g.L.ycge_render_frame_ansi_rgb_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, GAP, TOL, 0, p, cap, C.byref(n), info, None, None))
        return n.value
    fns = {"ansi": stream, "ansi delta": delta, "ansi rgb delta": rgb_delta}
    fns["_keep"] = out
    return fns


def layer_sets(g, count=4):
    """`count` arrangements that differ in their text row, as ctypes arrays ready for ycge_console_set_layers (the Python-side flattening is
    no part of what is timed)"""
    from yetanotherconsolegameengine_amd import abi
    from yetanotherconsolegameengine_amd.renderer import ConsoleLayer
    cw, ch = g.fbW + 1, g.fbH + 1
    sets = []
    for k in range(count):
        chars = np.full((ch, cw), 0x20, np.uint16)
        text = f"fps_{60 + k}___pos_{k}.{k}___the_quick_brown_fox_{'#' * (k + 1)}"
        chars[ch - 1, :len(text)] = [ord(c) for c in text]
        menu = np.full((10, 40), ord("."), np.uint16)
        menu[0], menu[-1] = ord("="), ord("=")
        layers = [ConsoleLayer(chars, (1.0, 1.0, 1.0), (0.0, 0.0, 0.5)), ConsoleLayer(menu, (1.0, 1.0, 0.0), (0.25, 0.25, 0.25), 100, 40)]
        arr = (abi.ConsoleLayer * 2)(*[l.as_struct() for l in layers])
        sets.append((arr, layers))
    return sets


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed(variants, rounds, frames):
    """variants: name -> (callable, counts as a delta).  Round by round, the order reversed on odd rounds; -> name -> ([ms per frame], bytes)"""
    names = list(variants)
    per, size = {v: [] for v in names}, {}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            fn = variants[v]
            fn()                          # (untimed: warms the variant's path after the others ran)
            t0 = time.perf_counter()
            for _ in range(frames):
                size[v] = fn()
            per[v].append((time.perf_counter() - t0) * 1e3 / frames)
    return per, size


def layered_against_unlayered(rounds, frames, settle):
    g0, g1, g2 = renderer(), renderer(), renderer()
    f0, f1, f2 = frame_fns(g0), frame_fns(g1), frame_fns(g2)
    sets = layer_sets(g1)
    g1._check(g1.L.ycge_console_set_layers(g1.ctx, sets[0][0], 2, 1))
    turn = [0]

    def set_then(fn):
        def run():
            turn[0] += 1
            g2._check(g2.L.ycge_console_set_layers(g2.ctx, sets[turn[0] % len(sets)][0], 2, 1))
            return fn()
        return run
    for f in (f0, f1, f2):
        for _ in range(settle):
            f["ansi delta"]()
    t0 = time.perf_counter()
    for k in range(20):
        g2._check(g2.L.ycge_console_set_layers(g2.ctx, sets[k % len(sets)][0], 2, 1))
    set_ms = (time.perf_counter() - t0) * 1e3 / 20
    res = {"layers": "a 1921 x 541 framebuffer below the raytrace one, blank but for one text row; a 40 x 10 framebuffer above at (100, 40)",
           "layer_cells": 1921 * 541 + 400, "set_call_ms_alone": set_ms, "rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle,
           "merge_gap": GAP, "tolerance": TOL, "calls": {}}
    for call in CALLS:
        per, size = timed({"none": f0[call], "layers": f1[call], "layers+set": set_then(f2[call])}, rounds, frames)
        ms = {v: stats(x) for v, x in per.items()}
        spread = ms["none"]["max"] - ms["none"]["min"]
        res["calls"][call] = {"ms_per_frame": ms, "bytes_a_frame": size, "spread_of_none_ms": spread,
                              "layers_minus_none_ms": ms["layers"]["median"] - ms["none"]["median"],
                              "layers_and_set_minus_none_ms": ms["layers+set"]["median"] - ms["none"]["median"],
                              "layers_within_spread": bool(abs(ms["layers"]["median"] - ms["none"]["median"]) <= spread)}
        print(call, json.dumps(res["calls"][call]), flush=True)
    for g in (g0, g1, g2):
        g.close()
    return res


def unlayered_against_parent(parent_lib, rounds, frames, settle):
    from yetanotherconsolegameengine_amd import abi
    P = abi.bind(C.CDLL(str(parent_lib)), names=[n for n in abi.EXPORTED_SYMBOLS if n != "ycge_console_set_layers"])
    assert not hasattr(P, "ycge_console_set_layers"), "the parent's library is expected to lack the export"
    ctxs = {"parent A": renderer(P), "product": renderer(), "parent B": renderer(P)}
    fns = {k: frame_fns(g) for k, g in ctxs.items()}
    for f in fns.values():
        for _ in range(settle):
            f["ansi delta"]()
    res = {"rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle, "calls": {}}
    for call in CALLS:
        per, size = timed({k: f[call] for k, f in fns.items()}, rounds, frames)
        parent = per["parent A"] + per["parent B"]
        spread = float(np.max(parent) - np.min(parent))
        diff = float(np.median(per["product"]) - np.median(parent))
        res["calls"][call] = {"ms_per_frame": {k: stats(v) for k, v in per.items()}, "bytes_a_frame": size, "parent_median_ms": float(np.median(parent)),
                              "parent_spread_ms": spread, "product_minus_parent_ms": diff, "agrees_within_the_parents_spread": bool(abs(diff) <= spread)}
        print("parent:", call, json.dumps(res["calls"][call]), flush=True)
    for g in ctxs.values():
        g.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames-per-round", type=int, default=10)
    ap.add_argument("--settle", type=int, default=40)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ansi_layers_rate.json"))
    a = ap.parse_args()
    m = {"what": "the layered ANSI streams on the device (ycge_console_set_layers) on one MI355X; profiles/ansi_layers_rate.py",
         "config": 4, "framebuffer": [1920, 540], "console": [1921, 541],
         "not_measured": "the terminal that consumes the bytes, the host that fills the framebuffers, and the C# wrappers (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    m["layered_against_unlayered"] = layered_against_unlayered(a.rounds, a.frames_per_round, a.settle)
    m["unlayered_against_parent"] = unlayered_against_parent(a.parent_lib, a.rounds, a.frames_per_round, a.settle) if a.parent_lib else "not measured"
    Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
