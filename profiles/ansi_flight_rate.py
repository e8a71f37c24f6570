"""ANSI streams with frames in flight (ycge_render_frame_async_ansi): the frame period of the four forms queued two at a time, against the
synchronous export of each form and against ycge_render_frame_async_chexels with the ANSI pairs alone (the same frame work and a 2.1 MB
read-back), in one process on one GPU.  The method of profiles/ansi_rgb_rate.py.

    python profiles/ansi_flight_rate.py --part rate --out DIR [--rounds 8 --frames 20 --parent-lib PATH]   the periods, at rest and moving
    python profiles/ansi_flight_rate.py --part kernel --out DIR       frames in flight and k_ansi_deliver through its hook (for rocprofv3 --kernel-trace)
    python profiles/ansi_flight_rate.py --part copies --out DIR       the synchronous forms (for a rocprofv3 --memory-copy-trace run of its own)
    python profiles/ansi_flight_rate.py --part merge --out DIR [--kernel-trace CSV --copy-trace CSV]     -> profiles/ansi_flight_rate.json

Config 4 at 1920 x 540 under a 1921 x 541 console, every destination page-locked memory of the library.  One context converges at rest
(60 frames); then the legs alternate round by round, in reversed order every other round: a round is 20 frames, the host clock around them,
the last call of the round a ycge_wait for the legs in flight.  A leg in flight queues two frames into two slots and waits, ten times a
round: two frames in flight, nothing else on the host between them.  `moving` repeats the rounds with the camera stepped before every
frame.  Behind another form the first delta call is a keyframe: one untimed frame leads every delta round.
Two expectations are written down with the numbers, not tuned for: the in-flight delta's period lies below the synchronous _ansi_delta of
the same run by more than that form's round-to-round spread (max - min), and within the async-chexels leg's own spread of that leg.
The kernel part runs k_ansi_deliver through ycge_test_ansi_deliver at one, two and four workgroups a CU for a full 256-colour stream's
size and a resting delta's, the three grids alternating launch by launch; the merge names the trace's launches by their order.
With --parent-lib, the parent commit's library (built elsewhere from the parent's sources) is loaded beside the product's, and two legs of
the parent and one of the product alternate round by round: in the first round the same frames at rest on each - the second call of each
synchronous form and of the delta in flight, its length and sha256 (`streams`) - and in every round the five legs in flight at rest
(`against_parent`, parent_check below).
Not measured: the terminal that consumes the bytes, and the C# wrapper (never compiled here).
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
for p in (str(ROOT), str(ROOT / "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

GAP = 3
FORMS = {"ansi": (False, False), "ansi delta": (False, True), "ansi rgb": (True, False), "ansi rgb delta": (True, True)}
LEGS = tuple(f"in flight {f}" for f in FORMS) + tuple(f"synchronous {f}" for f in FORMS) + ("in flight chexels ansi",)
FULL_BYTES, DELTA_BYTES = 3_100_000, 17_000          # a full 256-colour stream of the console and a resting delta, in round numbers (the hook's sizes)
TRACED, SETTLE_TRACED, HOOK_LAUNCHES = 20, 30, 12     # frames a traced leg runs, frames at rest before them, launches per hook setting


def renderer(lib=None):
    from yetanotherconsolegameengine_amd import scenes
    from yetanotherconsolegameengine_amd.renderer import RaytraceRenderer
    from yetanotherconsolegameengine_amd.scene import flatten
    sc, w, h, ss, pose = scenes.config_scene(4)
    g = RaytraceRenderer(flatten(sc), w, h, pose.get("fov", 45.0), ss, lib=lib)
    g.SetCamera(pose["pos"], pose["yaw"], pose["pitch"])
    return g, pose


def sync_call(g, form):
    """one synchronous frame of the form into the renderer's page-locked stream buffer (the raw export: no copy of the bytes on the host) -> length"""
    rgb, delta = FORMS[form]
    cw, ch = g.fbW + 1, g.fbH + 1
    out = g._ansi_out(cw, ch, True)
    p, cap, n = out.ctypes.data_as(C.POINTER(C.c_uint8)), g._ansi_bound(cw, ch, rgb, g.L), C.c_size_t(0)
    if rgb and delta:
        g._check(g.L.ycge_render_frame_ansi_rgb_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, GAP, 0, 0, p, cap, C.byref(n), None, None, None))
    elif delta:
        g._check(g.L.ycge_render_frame_ansi_delta(g.ctx, cw, ch, 0, 0, 7, 0, 0, GAP, 0, p, cap, C.byref(n), None, None, None))
    elif rgb:
        g._check(g.L.ycge_render_frame_ansi_rgb(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
    else:
        g._check(g.L.ycge_render_frame_ansi(g.ctx, cw, ch, 0, 0, 7, 0, 0, p, cap, C.byref(n), None, None))
    return n.value


def legs(g, pose, moving):
    """{leg: callable(frames) -> bytes of the last frame}; `moving` steps the camera before every frame"""
    cw, ch = g.fbW + 1, g.fbH + 1
    step = [0]

    def camera():
        if moving:
            step[0] += 1
            q, k = pose["pos"], step[0] % 200
            g.SetCamera((q[0] + 0.02 * k, q[1], q[2] - 0.01 * k), pose["yaw"] + 0.01 * k, pose["pitch"])

    def flight(form):
        rgb, delta = FORMS[form]

        def run(frames):
            for i in range(frames):
                camera()
                g.RenderAsyncAnsi(i % 2, cw, ch, rgb=rgb, delta=delta, merge_gap=GAP)
                if i % 2 == 1 or i == frames - 1:
                    g.Wait()
            return len(g.AsyncAnsiResult((frames - 1) % 2)[0])
        return run

    def sync(form):
        def run(frames):
            for _ in range(frames):
                camera()
                n = sync_call(g, form)
            return n
        return run

    def chexels(frames):
        for i in range(frames):
            camera()
            out = g.RenderAsyncChexels(i % 2, color16=False, ansi=True)
            if i % 2 == 1 or i == frames - 1:
                g.Wait()
        return out["ansi"].nbytes
    fns = {f"in flight {f}": flight(f) for f in FORMS}
    fns.update({f"synchronous {f}": sync(f) for f in FORMS})
    fns["in flight chexels ansi"] = chexels
    return fns


def rounds_of(g, pose, moving, rounds, frames):
    fns = legs(g, pose, moving)
    for leg in LEGS:
        fns[leg](4)
    per, size = {leg: [] for leg in LEGS}, {}
    for r in range(rounds):
        for leg in (LEGS if r % 2 == 0 else tuple(reversed(LEGS))):
            if "delta" in leg:
                fns[leg](1)              # (behind another form the first delta is a keyframe: not timed)
            t0 = time.perf_counter()
            size[leg] = fns[leg](frames)
            per[leg].append((time.perf_counter() - t0) * 1e3 / frames)
    ms = {leg: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for leg, v in per.items()}
    res = {"ms_per_frame": ms, "bytes_last_frame": size}
    sync_d, flight_d, chex = ms["synchronous ansi delta"], ms["in flight ansi delta"], ms["in flight chexels ansi"]
    res["in_flight_delta_below_synchronous_delta"] = {
        "gain_ms_median": sync_d["median"] - flight_d["median"], "synchronous_delta_spread_ms": sync_d["max"] - sync_d["min"],
        "holds": bool(sync_d["median"] - flight_d["median"] > sync_d["max"] - sync_d["min"])}
    res["in_flight_delta_within_chexels_leg"] = {
        "difference_ms_median": flight_d["median"] - chex["median"], "chexels_spread_ms": chex["max"] - chex["min"],
        "holds": bool(abs(flight_d["median"] - chex["median"]) <= chex["max"] - chex["min"])}
    return res


def parent_check(per):
    """per: (leg, form) -> [ms a frame of each round], the legs "parent A", "branch", "parent B" (two of the parent's, as
    profiles/ansi_layers_rate.py has them: what differs between two legs of ONE build is part of the noise) -> form -> the parent's median
    and spread (max - min) over the rounds of both its legs, each leg's median, and whether the branch's lies at or below the parent's
    median plus its spread.  Every round of a leg runs on a context of its own, the only one alive: a context's place among the live
    contexts of a process changes its period whichever library made it (of three, the second ran its frames in flight 0.25 ms slower
    and the third its synchronous frames 0.2 ms slower)"""
    res = {}
    for f in dict.fromkeys(f for _, f in per):
        p, b = per[("parent A", f)] + per[("parent B", f)], per[("branch", f)]
        res[f] = {"parent_median_ms": float(np.median(p)), "parent_spread_ms": float(np.max(p) - np.min(p)), "branch_median_ms": float(np.median(b)),
                  "branch_spread_ms": float(np.max(b) - np.min(b)), "parent_A_median_ms": float(np.median(per[("parent A", f)])),
                  "parent_B_median_ms": float(np.median(per[("parent B", f)]))}
        res[f]["within_allowance"] = bool(res[f]["branch_median_ms"] <= res[f]["parent_median_ms"] + res[f]["parent_spread_ms"])
    return res


def streams_at_rest(g):
    """on a context converged at rest: the second call of each synchronous form (behind another form the first delta is a keyframe), then of
    the delta in flight -> {form: [length, sha256]}"""
    import hashlib
    cw, ch = g.fbW + 1, g.fbH + 1
    res = {}
    for form in FORMS:
        sync_call(g, form)
        n = sync_call(g, form)
        res[f"synchronous {form}"] = [n, hashlib.sha256(g._ansi_out(cw, ch, True)[:n].tobytes()).hexdigest()]
    for slot in (0, 1):
        g.RenderAsyncAnsi(slot, cw, ch, delta=True, merge_gap=GAP)
        g.Wait()
    data = bytes(g.AsyncAnsiResult(1)[0])
    res["in flight ansi delta"] = [len(data), hashlib.sha256(data).hexdigest()]
    return res


def against_parent(parent_lib, rounds: int, frames: int, settle: int):
    from yetanotherconsolegameengine_amd import abi
    P = abi.load_library(parent_lib)
    libs = {"parent A": P, "branch": None, "parent B": P}
    flight = [leg for leg in LEGS if leg.startswith("in flight")]
    per, streams = {(b, leg): [] for b in libs for leg in flight}, {}
    for r in range(rounds):
        for b in (list(libs) if r % 2 == 0 else list(libs)[::-1]):
            g, pose = renderer(libs[b])
            for _ in range(settle):
                sync_call(g, "ansi delta")
            if r == 0:
                streams[b] = streams_at_rest(g)
            fns = legs(g, pose, False)
            for leg in flight:
                fns[leg](4)
            for leg in flight:
                if "delta" in leg:
                    fns[leg](1)          # (behind another form the first delta is a keyframe: not timed)
                t0 = time.perf_counter()
                fns[leg](frames)
                per[(b, leg)].append((time.perf_counter() - t0) * 1e3 / frames)
            g.close()
    return {"streams": dict(streams, equal_on_both_builds=streams["parent A"] == streams["branch"] == streams["parent B"]), "at_rest": parent_check(per)}


def part_rate(out: Path, rounds: int, frames: int, settle: int, parent_lib=None):
    g, pose = renderer()
    for _ in range(settle):              # the camera rests: TAA converges
        sync_call(g, "ansi delta")
    res = {"rounds": rounds, "frames_per_round": frames, "frames_at_rest_before": settle, "merge_gap": GAP, "frames_in_flight": 2,
           "at_rest": rounds_of(g, pose, False, rounds, frames)}
    res["moving"] = rounds_of(g, pose, True, rounds, frames)
    res["device"] = str(g.device_info())
    g.close()
    if parent_lib:
        res["against_parent"] = against_parent(parent_lib, rounds, frames, settle)
    print(json.dumps(res), flush=True)
    (out / "rate.json").write_text(json.dumps(res, indent=1))


def part_kernel(out: Path):
    """for rocprofv3 --kernel-trace: 20 full 256-colour frames and 20 resting deltas in flight, then the hook at 1, 2 and 4 workgroups a CU"""
    from yetanotherconsolegameengine_amd import abi
    g, pose = renderer()
    fns = legs(g, pose, False)
    for _ in range(SETTLE_TRACED):
        sync_call(g, "ansi delta")
    sizes = {"in flight ansi": fns["in flight ansi"](TRACED)}
    fns["in flight ansi delta"](1)
    sizes["in flight ansi delta"] = fns["in flight ansi delta"](TRACED)
    fn = g.L.ycge_test_ansi_deliver
    fn.restype, fn.argtypes = abi.ANSI_FLIGHT_HOOK_PROTOTYPES["ycge_test_ansi_deliver"]
    cus = int(g.device_info()[1]) if isinstance(g.device_info(), (tuple, list)) else 0
    dst = g._page_locked_zeros((FULL_BYTES + 64,), np.uint8)[0]
    rec = g._page_locked_zeros((32,), np.uint8)[0]
    src = np.random.default_rng(1).integers(0, 256, FULL_BYTES, dtype=np.uint8)
    plan = []                            # launch by launch; the three grids alternate, the first of them rotating, so that none is always the first
    for n in (FULL_BYTES, DELTA_BYTES):
        for k in range(HOOK_LAUNCHES + 2):
            for j in range(3):
                factor = (1, 2, 4)[(j + k) % 3]
                groups = cus * factor if cus > 0 else 0
                g._check(fn(g.ctx, src.ctypes.data, n, n, FULL_BYTES, 0, (C.c_uint32 * 3)(), groups, dst.ctypes.data, rec.ctypes.data))
                plan.append({"bytes": n, "workgroups": groups, "per_cu": factor, "warm_up": k < 2})
    g.close()
    (out / "kernel_plan.json").write_text(json.dumps({"compute_units": cus, "frames": sizes, "hook": plan}, indent=1))


def part_copies(out: Path):
    """for a rocprofv3 --memory-copy-trace run of its own: the synchronous forms' exact-length copies"""
    g, _ = renderer()
    for _ in range(SETTLE_TRACED):
        sync_call(g, "ansi delta")
    sizes = {}
    for form in ("ansi", "ansi delta"):
        sync_call(g, form)               # (the delta behind the full streams: a keyframe)
        for _ in range(TRACED):
            sizes[form] = sync_call(g, form)
    g.close()
    (out / "copies_plan.json").write_text(json.dumps(sizes, indent=1))


def _col(row, *names):
    for n in names:
        if n in row and row[n] not in ("", None):
            return row[n]
    return None


def _us(r):
    return (int(_col(r, "End_Timestamp")) - int(_col(r, "Start_Timestamp"))) / 1e3


def _stats(v):
    return {"calls": len(v), "median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))} if v else {"calls": 0}


def deliver_rows(path, plan):
    """k_ansi_deliver's launches of a rocprofv3 --kernel-trace CSV in launch order, named by what part_kernel ran: the frames in flight (full
    streams, the delta leg's leading keyframe, resting deltas), then the hook's settings"""
    rows = sorted((r for r in csv.DictReader(open(path)) if "k_ansi_deliver" in (_col(r, "Kernel_Name", "Name") or "")), key=lambda r: int(_col(r, "Start_Timestamp")))
    names = [f"frame in flight, full 256-colour stream ({plan['frames']['in flight ansi']} bytes)"] * TRACED + ["frame in flight, keyframe"] + \
            [f"frame in flight, resting delta ({plan['frames']['in flight ansi delta']} bytes)"] * TRACED
    names += [None if h["warm_up"] else f"hook, {h['bytes']} bytes, {h['workgroups']} workgroups ({h['per_cu']} a CU)" for h in plan["hook"]]
    if len(rows) != len(names):
        return {"error": f"{len(rows)} launches in the trace, {len(names)} expected"}
    by = {}
    for r, n in zip(rows, names):
        if n is None:
            continue
        assert "hook" not in n or int(_col(r, "Grid_Size_X", "Grid_Size")) == 256 * int(n.split(" bytes, ")[1].split(" ")[0]), (n, r)
        by.setdefault(n, []).append(_us(r))
    return [dict(what=n, **_stats(v)) for n, v in by.items()]


def copy_rows(path, plan):
    """the device-to-host copies of a rocprofv3 --memory-copy-trace CSV in order, named by what part_copies ran (the trace carries no byte
    count): one exact-length copy a synchronous frame - the settling deltas, the full streams, the delta leg's keyframe, the resting deltas"""
    rows = sorted((r for r in csv.DictReader(open(path)) if "DEVICE_TO_HOST" in (_col(r, "Direction") or "")), key=lambda r: int(_col(r, "Start_Timestamp")))
    us = [_us(r) for r in rows]
    a, b = SETTLE_TRACED, SETTLE_TRACED + 1 + TRACED
    return {"copies_in_trace": len(us), "copies_expected": SETTLE_TRACED + 2 * (1 + TRACED),
            f"synchronous _ansi, full 256-colour stream ({plan['ansi']} bytes)": _stats(us[a:b]),
            f"synchronous _ansi_delta, resting delta ({plan['ansi delta']} bytes)": _stats(us[b + 1:])}


def part_merge(out: Path, kernel_trace, copy_trace):
    m = {"what": "ANSI streams with frames in flight (ycge_render_frame_async_ansi) on one MI355X; profiles/ansi_flight_rate.py",
         "config": 4, "framebuffer": [1920, 540], "console": [1921, 541],
         "not_measured": "the terminal that consumes the bytes, and the C# wrapper (never compiled here)"}
    try:
        from yetanotherconsolegameengine_amd import build
        m["build"] = build.source_hash()
    except Exception:
        pass
    for part in ("rate", "kernel_plan", "copies_plan"):
        p = out / f"{part}.json"
        m[part] = json.loads(p.read_text()) if p.exists() else "not_measured"
    have = lambda f, part: f and Path(f).exists() and isinstance(m[part], dict)
    m["k_ansi_deliver_rocprofv3"] = deliver_rows(kernel_trace, m["kernel_plan"]) if have(kernel_trace, "kernel_plan") else "not_measured"
    m["synchronous_copies_rocprofv3"] = copy_rows(copy_trace, m["copies_plan"]) if have(copy_trace, "copies_plan") else "not_measured"
    (ROOT / "profiles" / "ansi_flight_rate.json").write_text(json.dumps(m, indent=1) + "\n")
    print(json.dumps(m)[:6000])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("rate", "kernel", "copies", "merge"), required=True)
    ap.add_argument("--out", required=True, help="directory for the parts' JSON (outside the tree, or one git ignores)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--settle", type=int, default=60)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--copy-trace", default=None)
    ap.add_argument("--parent-lib", default=None, help="rate: the parent commit's library, measured beside the product's")
    a = ap.parse_args()
    out = Path(a.out); out.mkdir(parents=True, exist_ok=True)
    if a.part == "rate": part_rate(out, a.rounds, a.frames, a.settle, a.parent_lib)
    elif a.part == "kernel": part_kernel(out)
    elif a.part == "copies": part_copies(out)
    else: part_merge(out, a.kernel_trace, a.copy_trace)
