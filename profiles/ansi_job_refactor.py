"""The ANSI stream calls through this build against the parent commit's library: host code only, so every form is expected where it was.

    python profiles/ansi_job_refactor.py --parent-lib PATH --out FILE [--rounds 8 --frames 20 --settle 60]

The unlayered forms and the frames in flight are ansi_rgb_rate.py's and ansi_flight_rate.py's own --parent-lib parts.  The layered and the
quadrant forms are measured here in the same way - two legs of the parent and one of the branch alternate round by round, every round of a
leg on a context of its own, the only one alive - with those scripts' frames: their own --parent-lib parts compare the calls a parent
WITHOUT layers or quadrants also has.  Per form: the parent's median and spread (max - min) over the rounds of both its legs, the branch's
median, and whether it lies at or below the parent's median plus that spread; and [length, sha256] of the second call at rest on every leg.
"""
import argparse
import hashlib
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (str(ROOT), str(ROOT / "tests"), str(ROOT / "profiles")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ansi_flight_rate as F
import ansi_layers_rate as L
import ansi_rgb_rate as R
import quadrant_rate as Q


def legs_of(parent_lib, rounds, frames, settle, calls, make):
    """make(lib) -> (context, {call: callable returning the stream's length}, the page-locked stream buffer, the call to settle with)"""
    from yetanotherconsolegameengine_amd import abi
    P = abi.load_library(parent_lib)
    libs = {"parent A": P, "branch": None, "parent B": P}
    per, streams = {(b, c): [] for b in libs for c in calls}, {b: {} for b in libs}
    for r in range(rounds):
        for b in (list(libs) if r % 2 == 0 else list(libs)[::-1]):
            g, fns, out, rest = make(libs[b])
            for _ in range(settle):
                fns[rest]()
            for c in calls:
                fns[c]()                  # (behind another form the first delta call is a keyframe: not timed)
                n = fns[c]()
                if r == 0:
                    streams[b][c] = [n, hashlib.sha256(out[:n].tobytes()).hexdigest()]
                t0 = time.perf_counter()
                for _ in range(frames):
                    fns[c]()
                per[(b, c)].append((time.perf_counter() - t0) * 1e3 / frames)
            g.close()
    return {"streams": dict(streams, equal_on_both_builds=streams["parent A"] == streams["branch"] == streams["parent B"]), "at_rest": R.parent_check(per)}


def layered(layer_set):
    def make(lib):
        g = L.renderer(lib)
        g._check(g.L.ycge_console_set_layers(g.ctx, layer_set, 2, 1))
        fns = L.frame_fns(g)
        return g, fns, fns["_keep"], "ansi delta"
    return make


def quadrants(lib):
    g = Q.renderer(4, lib)
    fns = Q.frame_fns(g)
    return g, fns, fns["_keep"][0], "ansi quad delta"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--settle", type=int, default=60)
    a = ap.parse_args()
    from yetanotherconsolegameengine_amd import build
    m = {"branch_source_hash": build.source_hash(), "rounds": a.rounds, "frames_per_round": a.frames, "frames_at_rest_before": a.settle,
         "frame_check": "per form, branch median <= parent median + parent (max - min) over the rounds of both its legs"}
    probe = L.renderer()
    layer_set = L.layer_sets(probe, 1)[0]          # (the ctypes array and the layers that own its cells)
    probe.close()
    parts = (("synchronous_ansi", lambda: R.rate_against_parent(a.parent_lib, a.rounds, a.frames, a.settle)),
             ("in_flight", lambda: F.against_parent(a.parent_lib, a.rounds, a.frames, a.settle)),
             ("layered", lambda: legs_of(a.parent_lib, a.rounds, a.frames, a.settle, L.CALLS, layered(layer_set[0]))),
             ("quadrants", lambda: legs_of(a.parent_lib, a.rounds, a.frames, a.settle, ("ansi quad", "ansi quad delta"), quadrants)))
    for name, run in parts:
        m[name] = run()
        print(name, json.dumps(m[name]), flush=True)
        Path(a.out).write_text(json.dumps(m, indent=1) + "\n")
