"""Video mode on the device (ycge_video_blit / ycge_video_blit_ansi): what one blit of a 1920 x 1080 BGR frame costs for each destination
set, against the frame's own trip over the link.  One GPU, one process.

    python profiles/video_rate.py --part rate   --out DIR [--rounds R --calls K]   ms per call of each form, ss 1 and ss 2 -> DIR/rate.json
    python profiles/video_rate.py --part kernel --out DIR --ss K                   a short run of one geometry (for rocprofv3 -d DIR/prof_ss<K>)
    python profiles/video_rate.py --part merge  --out DIR                          rate.json, prof_ss*/, bench_{branch,parent}_*.log -> profiles/video_rate.json

Geometries: 1920 x 1080 x 3 -> 1920 x 540 chexels at ss 1 (hi-res 1920 x 1080, scale 1) and at ss 2 (hi-res 3840 x 2160, scale 2).
Forms, alternated round by round: `sdr` the SDR array alone (24 bytes a chexel back), `color16` one byte a chexel, `ansi stream`
ycge_video_blit_ansi for a console one cell wider and taller than the framebuffer.  The source frame and every destination are
page-locked memory of the library; a call's time is the host clock around it (it returns with the bytes in the caller's memory).
`upload` is the floor stated beside them: the same src_w * src_h * 3 bytes from page-locked memory to the device, one synchronous
hipMemcpy through torch, measured in the same run.  The kernel's own time comes from a separate
`rocprofv3 --kernel-trace --stats -- python profiles/video_rate.py --part kernel --ss K` run per geometry, whose kernel_stats.csv the
merge reads; `bench_ab` is read from the logs of plain bench.py runs on this branch and with the parent's library.
Not measured: the host time of VideoRenderer.TryFlipAndBlit under .NET (no toolchain).
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

SRC_W, SRC_H, BPP, FB_W, FB_H = 1920, 1080, 3, 1920, 540
FORMS = ("sdr", "color16", "ansi stream")
U8P = C.POINTER(C.c_uint8)


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def setup(ss):
    from yetanotherconsolegameengine_amd.renderer import VideoRenderer
    v = VideoRenderer(FB_W, FB_H, ss)
    r = v._r
    frame = r._page_locked_zeros((SRC_H, SRC_W, BPP), np.uint8)[0]
    frame[...] = np.random.default_rng(1).integers(0, 256, frame.shape, dtype=np.uint8)
    shapes = r.chexel_shapes()
    sdr = r._page_locked_zeros(*shapes["sdr"])[0]
    c16 = r._page_locked_zeros(*shapes["color16"])[0]
    cw, ch = FB_W + 1, FB_H + 1
    cap = r.ansi_stream_bound(cw, ch, r.L)
    stream = r._page_locked_zeros((cap,), np.uint8)[0]
    n = C.c_size_t(0)
    fp = frame.ctypes.data_as(U8P)
    L, ctx = v.L, v.ctx

    def f_sdr():
        r._check(L.ycge_video_blit(ctx, fp, SRC_W, SRC_H, BPP, sdr.ctypes.data_as(C.POINTER(C.c_float)), None, None, None))
        return sdr.nbytes

    def f_c16():
        r._check(L.ycge_video_blit(ctx, fp, SRC_W, SRC_H, BPP, None, c16.ctypes.data_as(U8P), None, None))
        return c16.nbytes

    def f_ansi():
        r._check(L.ycge_video_blit_ansi(ctx, fp, SRC_W, SRC_H, BPP, cw, ch, 0, 0, 7, 0, 0, stream.ctypes.data_as(U8P), cap, C.byref(n), None))
        return n.value

    return v, frame, {"sdr": f_sdr, "color16": f_c16, "ansi stream": f_ansi}, (sdr, c16, stream)


def part_rate(out: Path, rounds: int, calls: int):
    import torch
    res = {"source": [SRC_W, SRC_H, BPP], "framebuffer": [FB_W, FB_H], "rounds": rounds, "calls_per_round": calls, "bytes_up": SRC_W * SRC_H * BPP, "geometries": {}}
    host = torch.empty(SRC_W * SRC_H * BPP, dtype=torch.uint8).pin_memory()
    dev = torch.empty_like(host, device="cuda")
    for ss in (1, 2):
        v, frame, fns, keep = setup(ss)
        for fn in fns.values():          # warm-up: tables, buffers, code objects
            for _ in range(3):
                fn()
        ms = {k: [] for k in FORMS + ("upload",)}
        back = {}
        for _ in range(rounds):
            for form in FORMS:
                t0 = time.perf_counter()
                for _ in range(calls):
                    back[form] = fns[form]()
                ms[form].append((time.perf_counter() - t0) * 1e3 / calls)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                dev.copy_(host)
                torch.cuda.synchronize()
            ms["upload"].append((time.perf_counter() - t0) * 1e3 / calls)
        res["geometries"][f"ss{ss}"] = {"hi_res": [FB_W * ss, FB_H * 2 * ss], "ms_per_call": {k: stats(x) for k, x in ms.items()}, "bytes_back": back}
        v.close()
    res["device"] = torch.cuda.get_device_name(0)
    (out / "rate.json").write_text(json.dumps(res, indent=1))
    print(json.dumps(res["geometries"]))


def part_kernel(out: Path, ss: int):
    v, frame, fns, keep = setup(ss)
    for _ in range(40):
        fns["sdr"]()
    v.close()


def bench_runs(logs):
    """the JSON result line of each bench.py log: its headline"""
    runs = []
    for f in logs:
        for line in reversed(Path(f).read_text().splitlines()):
            if line.startswith("{"):
                d = json.loads(line)
                runs.append({k: d[k] for k in ("value", "unit", "metric", "Mrays_s", "ms_per_step") if k in d})
                break
    return runs


def part_merge(out: Path):
    res = json.loads((out / "rate.json").read_text())
    kern = {}
    for ss in (1, 2):          # one rocprofv3 run per geometry: DIR/prof_ss<k>/**/*kernel_stats.csv
        for f in sorted((out / f"prof_ss{ss}").rglob("*kernel_stats.csv")):
            for row in csv.DictReader(open(f)):
                if "k_video_blit" in row.get("Name", ""):
                    kern[f"ss{ss}"] = {"calls": int(row["Calls"]), "mean_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    res["kernel"] = dict(kern, source="rocprofv3 --kernel-trace --stats, one run of its own per geometry (43 blits each, warm-up included)") if kern else "not_measured"
    branch, parent = bench_runs(sorted(out.glob("bench_branch_*.log"))), bench_runs(sorted(out.glob("bench_parent_*.log")))
    res["not_measured"] = ["the host time of VideoRenderer.TryFlipAndBlit under .NET (no toolchain)"] + ([] if branch and parent else ["bench_ab"])
    if branch and parent:
        res["bench_ab"] = {"what": "plain `bench.py --gpus 1`, branch and parent alternated in one job on one MI355X; the parent through its own library (YCGE_LIB)",
                           "branch": branch, "parent": parent}
    (ROOT / "profiles" / "video_rate.json").write_text(json.dumps(res, indent=1) + "\n")
    print("wrote profiles/video_rate.json")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["rate", "kernel", "merge"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ss", type=int, default=1)
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    if a.part == "rate":
        part_rate(out, a.rounds, a.calls)
    elif a.part == "kernel":
        part_kernel(out, a.ss)
    else:
        part_merge(out)
