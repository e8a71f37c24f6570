"""CPU search for the small windows tests/test_worldpregen_cpu.py pins (WINDOWS there): origins and seeds at which the restatement of
GenerateAndSaveWorld (tests/worldpregen_restatement.py) shows what the tests want to see.  Near the origin the reference's world is
almost all lake at small world heights, so the search looks elsewhere.

    python profiles/worldpregen_windows.py [--budget SECONDS]

For each configuration (chunk size, chunks_y, chunks_x, chunks_z, seed) it classifies a coarse grid of the island from the noise-only
fields (slope taken as 0), keeps the points that promise forest, desert or coast, evaluates the windows centred there and tags them;
it prints, tag by tag, the first window found that carries it, and stops when every tag has one or the budget is spent.
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
import worldgen_restatement as R          # noqa: E402
import worldpregen_restatement as P       # noqa: E402

F = np.float32
TAGS = P.TAGS
CONFIGS = [  # (S, chunks_y, chunks_x, chunks_z, seed).  World heights of 48 and below were tried (chunks_y = 3..6 at these sizes, seeds 0..6):
    # no point of a 125-block grid over the island is land more than 2 above the sea there (candidates() found none) - LocalWaterY's lakes
    # start 8 above the sea and cover all higher ground - so no tree meets the clip at the world's top (FloraPlacer.cs:168-169), which
    # needs ground within 16 of the top
    (16, 8, 4, 4, 0), (12, 10, 5, 4, 0), (8, 16, 6, 6, 0), (12, 10, 3, 3, 7), (8, 14, 5, 4, 3),
]


def candidates(cfg, stride=125):
    """Window centres that promise something, most promising first: coarse classification from the noise-only fields."""
    n = int(21000 // stride)
    xs = (np.arange(n) * stride - 10500).astype(np.int64)
    gx, gz = np.meshgrid(xs, xs, indexing="ij")
    ground = R.height_y(gx, gz, cfg)
    fx, fz = gx.astype(F), gz.astype(F)
    dry = F(0.55) * R.ridged2(fx * F(0.0020), fz * F(0.0020), 4, cfg.seed + 5003) + F(0.45) * (F(1) - R.fbm2(fx * F(0.0025), fz * F(0.0025), 5, cfg.seed + 5002))
    water = R.local_water_y(gx, gz, cfg, ground, np.zeros_like(fx))
    land = (ground > water) & (ground > cfg.sea + 2)
    score = land.astype(np.int64) * (1 + (dry > F(0.52)) + 2 * (ground + 16 >= cfg.height))
    order = np.argsort(-score, axis=None, kind="stable")
    inland = [(int(gx.flat[i]), int(gz.flat[i])) for i in order if score.flat[i] > 0]
    sea = ground <= cfg.sea - 1          # the shore: a sea point with land within two grid steps
    near = np.zeros_like(land)
    for sx in range(-2, 3):
        for sz in range(-2, 3):
            near |= np.roll(np.roll(land, sx, 0), sz, 1)
    shore = [(int(gx[i, j]), int(gz[i, j])) for i, j in zip(*np.nonzero(sea & near))]
    out = []
    for k in range(max(len(inland), len(shore))):          # three inland centres, then one at the shore
        out += inland[3 * k:3 * k + 3] + shore[k:k + 1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--budget", type=float, default=600.0)
    ap.add_argument("--per-config", type=int, default=40)
    ap.add_argument("--all", action="store_true", help="print every window looked at, not only those that bring a new tag")
    args = ap.parse_args()
    t0 = time.time()
    found = {}
    for S, cy, cx, cz, seed in CONFIGS:
        cfg = R.Config(S, cy, seed)
        cand = candidates(cfg)
        print(f"# S={S} chunks_y={cy} {cx}x{cz} seed={seed}: {len(cand)} candidate centres", flush=True)
        for k, (px, pz) in enumerate(cand[:args.per_config]):
            if time.time() - t0 > args.budget or (len(found) == len(TAGS) and not args.all):
                break
            ox, oz = px - cx * S // 2, pz - cz * S // 2
            tg = P.window_tags(cfg, *P.generate_world(cfg, cx, cz, ox, oz), ox, oz)
            new = [t for t in tg if t not in found]
            for t in new:
                found[t] = (S, cy, cx, cz, seed, ox, oz)
            if new or args.all:
                print(f"window S={S} chunks_y={cy} chunks=({cx},{cz}) seed={seed} origin=({ox},{oz}): {sorted(tg)}  NEW {sorted(new)}", flush=True)
    print("# tags without a window:", [t for t in TAGS if t not in found])
    for t in TAGS:
        if t in found:
            print(t, found[t])


if __name__ == "__main__":
    main()
