"""A numpy-float32 restatement of WorldManager.GenerateAndSaveWorld (reference Scenes/WorldGeneration/WorldManager.cs:510-631,
RiverNetworkGlobal.cs, FloraPlacer.PlaceTreesGlobal), written from the C# and not from csrc/ycge_worldgen.h: what
tests/test_worldpregen_cpu.py holds ycge_worldgen_world_cells to.

The noise functions are tests/worldgen_restatement.py's.  The river pass is the literal loop over a real ascending sort; the flora pass is
the literal serial loops.  The one addition is the origin: column (x, z) of the window is block (ox + x, oz + z) wherever the C# hands a
coordinate to a noise, hash or strata function; every bound and clamp stays the window's.
"""
import math

import numpy as np

import worldgen_restatement as R
from worldgen_restatement import AIR, DESERT, F, FOREST, LAKES, LEAVES, OCEAN, STONE, TALLGRASS, WOOD, BEACH  # noqa: F401

BEACH_BUFFER, RIVER_BANK_SAND = 2, F(1.5)          # IslandSettings.cs:10, :54


def d8_global(ground):          # RiverNetworkGlobal.cs:17-40
    nx, nz = ground.shape
    dnx, dnz, best = np.zeros((nx, nz), np.int64), np.zeros((nx, nz), np.int64), np.zeros((nx, nz), np.int64)
    big = np.iinfo(np.int64).max // 4
    pad = np.full((nx + 2, nz + 2), big, np.int64)          # a neighbour outside the window is skipped: its drop is never > best
    pad[1:-1, 1:-1] = ground
    for oz in (-1, 0, 1):
        for ox in (-1, 0, 1):
            if ox == 0 and oz == 0:
                continue
            drop = ground - pad[1 + ox:nx + 1 + ox, 1 + oz:nz + 1 + oz]
            better = drop > best
            best = np.where(better, drop, best); dnx = np.where(better, ox, dnx); dnz = np.where(better, oz, dnz)
    return dnx, dnz


def accum_sorted(ground, dnx, dnz, reverse_ties=False):
    """RiverNetworkGlobal.cs:42-63, literally.  Array.Sort is unstable: reverse_ties visits equal heights in the opposite index order."""
    nx, nz = ground.shape
    order = [(x, z, int(ground[x, z])) for x in range(nx) for z in range(nz)]
    if reverse_ties:
        order.reverse()
    order.sort(key=lambda c: c[2])
    accum = np.zeros((nx, nz), F)
    for x, z, _ in order:
        a = accum[x, z]
        if a <= 0:
            a = F(1.0)
        x2, z2 = x + int(dnx[x, z]), z + int(dnz[x, z])
        if dnx[x, z] != 0 or dnz[x, z] != 0:
            if 0 <= x2 < nx and 0 <= z2 < nz:
                accum[x2, z2] += a
    return accum


def carve_global(accum, ground, sea):          # RiverNetworkGlobal.cs:65-83, WorldManager.cs:536
    t = (np.asarray(accum, F) - F(50)) / F(50)
    carve = np.where(t <= 0, F(0), np.minimum(F(3.5), np.maximum(F(0), t) * F(3.5))).astype(F)
    river_water = np.where(t <= 0, sea, np.maximum(sea, ground - np.floor(carve).astype(np.int64) + int(math.ceil(2.0))))
    return np.maximum(0, ground - np.floor(carve).astype(np.int64)), river_water


def noise_fields(cfg, nx, nz, ox=0, oz=0):
    """What depends on the block coordinates alone: HeightY, BiomeMap's dryness verdict, StrataMap's noise."""
    x, z = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    gx, gz = ox + x, oz + z
    fx, fz = gx.astype(F), gz.astype(F)
    m1 = R.fbm2(fx * F(0.0025), fz * F(0.0025), 5, cfg.seed + 5002)
    r1 = R.ridged2(fx * F(0.0020), fz * F(0.0020), 4, cfg.seed + 5003)
    dry = F(0.55) * r1 + F(0.45) * (F(1) - m1)
    rock_n = R.fbm2(fx * F(0.004), fz * F(0.004), 3, cfg.seed + 4201)
    return dict(gx=gx, gz=gz, ground0=R.height_y(gx, gz, cfg), climate=np.where(dry > F(0.52), DESERT, FOREST), rock_n=rock_n,
                rock=np.where(rock_n < F(0.33), 0, np.where(rock_n < F(0.66), 1, 2)))


def fields(cfg, nx, nz, ox=0, oz=0, accum_fn=accum_sorted):
    """WorldManager.cs:521-560."""
    f = noise_fields(cfg, nx, nz, ox, oz)
    dnx, dnz = d8_global(f["ground0"])
    accum = accum_fn(f["ground0"], dnx, dnz)
    ground, river_water = carve_global(accum, f["ground0"], cfg.sea)
    ix, iz = np.arange(nx), np.arange(nz)
    dx = (ground[np.minimum(nx - 1, ix + 1), :] - ground[np.maximum(0, ix - 1), :]).astype(F) * F(0.5)
    dz = (ground[:, np.minimum(nz - 1, iz + 1)] - ground[:, np.maximum(0, iz - 1)]).astype(F) * F(0.5)
    slope = R.saturate(np.sqrt(dx * dx + dz * dz) / F(6))
    biome = np.where(ground <= cfg.sea - 1, OCEAN, np.where(np.abs(ground - cfg.sea) <= BEACH_BUFFER, BEACH, f["climate"]))
    water = np.maximum(R.local_water_y(f["gx"], f["gz"], cfg, ground, slope), river_water)
    biome = np.where((water > cfg.sea) & (ground <= water), LAKES, biome)
    f.update(dnx=dnx, dnz=dnz, dir=(dnx + 1) * 3 + (dnz + 1), accum=accum, ground=ground, river_water=river_water, slope=slope, biome=biome, water=water)
    return f


def fill(cfg, f):
    """WorldManager.cs:562-601 -> int32 [nx, ny, nz, 2]"""
    nx, nz = f["ground"].shape
    ny = cfg.height
    cells = np.zeros((nx, ny, nz, 2), np.int32)
    gy = np.arange(ny)[None, :, None]
    gY, wY = f["ground"][:, None, :], f["water"][:, None, :]
    biome, slope = f["biome"][:, None, :], f["slope"][:, None, :]
    surface = np.where(gY >= cfg.snow, R.SNOW, np.where(np.abs(gY - cfg.sea) <= 2, R.SAND, np.where(slope > F(0.80), STONE, np.where(biome == DESERT, R.SAND, R.GRASS))))
    surface = np.where((wY > cfg.sea) & ((wY - gY).astype(F) <= F(BEACH_BUFFER) + RIVER_BANK_SAND), R.SAND, surface)          # :580
    sub = np.where(gY <= cfg.sea + 1, R.SAND, np.where(biome == DESERT, R.SAND, np.where(gY - gy <= 3, R.DIRT, STONE)))
    mat = np.where(gy > gY, np.where(gy <= wY, R.WATER, AIR), np.where(gy == gY, surface, np.where(gy >= gY - 3, sub, STONE)))
    band = (np.fmod(gy, 24)).astype(F) / F(24)
    base_meta = np.where(band < F(0.33), 0, np.where(band < F(0.66), 1, 2))
    n = f["rock_n"][:, None, :]
    meta = np.where(n < F(0.33), 0, np.where(n < F(0.66), 1, base_meta))
    cells[..., 0] = mat
    cells[..., 1] = np.where(gy < gY - 3, meta, 0)
    return cells


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def place_trees_global(cfg, f, cells, ox=0, oz=0):
    """FloraPlacer.cs:137-254, loop for loop, on `cells` in place.  Returns what it placed, for the tests to look at:
    trees [(gx, gz, conifer, trunkBase, trunkH, canopyR, clipped at the top, anyLeaves)], cacti [(gx, gz, height)], rocks [(gx, gz)]."""
    ground, biome, slope, water = f["ground"], f["biome"], f["slope"], f["water"]
    nx, nz = ground.shape
    ny, snow = cfg.height, cfg.snow
    trees, cacti, rocks = [], [], []
    for gx in range(nx):
        for gz in range(nz):
            gY, wY = int(ground[gx, gz]), int(water[gx, gz])
            if gY <= wY or gY >= snow - 2:
                continue
            if biome[gx, gz] != FOREST:
                continue
            h = R.flora_hash(ox + gx, oz + gz, cfg.seed + 90001)
            if F(h & 0xFFFF) / F(65535.0) > F(0.03):
                continue
            conifer = ((h >> 16) & 3) == 0
            base = gY + 1
            th = 6 + ((h >> 2) & 7) if conifer else 4 + ((h >> 3) & 5)
            r = 2 if conifer else 2 + ((h >> 6) & 1)
            clipped = base + th + 2 >= ny
            if clipped:
                th = max(3, ny - base - 2)
            for t in range(th):
                y = base + t
                if y < 0 or y >= ny:
                    break
                if cells[gx, y, gz, 0] in (AIR, TALLGRASS):
                    cells[gx, y, gz] = (WOOD, 0)
            cbase, any_leaves = base + th - (2 if conifer else 1), False
            for dy in range(0 if conifer else -1, 3):
                y = cbase + dy
                if y < 0 or y >= ny:
                    continue
                rad = max(1, r - abs(dy)) if conifer else r - (1 if dy == 2 else 0)
                for rx in range(-rad, rad + 1):
                    x2 = gx + rx
                    if x2 < 0 or x2 >= nx:
                        continue
                    for rz in range(-rad, rad + 1):
                        z2 = gz + rz
                        if z2 < 0 or z2 >= nz:
                            continue
                        if cells[x2, y, z2, 0] in (AIR, TALLGRASS):
                            cells[x2, y, z2] = (LEAVES, 0); any_leaves = True
            if not any_leaves:
                y = base + th - 1
                if 0 <= y < ny:
                    for rx in (-1, 0, 1):
                        for rz in (-1, 0, 1):
                            x2, z2 = gx + rx, gz + rz
                            if 0 <= x2 < nx and 0 <= z2 < nz and cells[x2, y, z2, 0] == AIR:
                                cells[x2, y, z2] = (LEAVES, 0)
            trees.append((gx, gz, conifer, base, th, r, clipped, any_leaves))
        for gz in range(nz):
            if biome[gx, gz] != DESERT:
                continue
            gY, wY = int(ground[gx, gz]), int(water[gx, gz])
            if gY <= wY or slope[gx, gz] > F(0.25):
                continue
            bx, bz = ox + gx, oz + gz
            h = R.flora_hash(_i32(_i32(bx * 73856093) ^ _i32(bz * 19349663)), _i32(_i32(bz * 83492791) ^ _i32(bx * 297121507)), cfg.seed + 1234567)
            r = F(h & 0xFFFF) / F(65535.0)
            if r < F(0.70):
                continue
            if r < F(0.85):
                height = 2 + ((h >> 16) & 3)
                for t in range(1, height + 1):
                    y = gY + t
                    if y >= ny:
                        break
                    if cells[gx, y, gz, 0] == AIR:
                        cells[gx, y, gz] = (WOOD, 0)
                cacti.append((gx, gz, height))
            else:
                y = gY + 1
                if y >= ny:
                    continue
                for rx in (-1, 0, 1):
                    for rz in (-1, 0, 1):
                        x2, z2 = gx + rx, gz + rz
                        if 0 <= x2 < nx and 0 <= z2 < nz and abs(rx) + abs(rz) <= 1 and cells[x2, y, z2, 0] == AIR:
                            cells[x2, y, z2] = (STONE, 1)
                rocks.append((gx, gz))
    return dict(trees=trees, cacti=cacti, rocks=rocks)


def generate_world(cfg, chunks_x, chunks_z, ox=0, oz=0):
    """-> (cells int32 [nx, ny, nz, 2], fields, placed)"""
    f = fields(cfg, chunks_x * cfg.size, chunks_z * cfg.size, ox, oz)
    cells = fill(cfg, f)
    placed = place_trees_global(cfg, f, cells, ox, oz)
    return cells, f, placed


def chunk_occupied(cells, S):
    """AttachChunkFromPreloaded's anySolid (WorldManager.cs:704-720) per chunk -> bool [chunks_x, chunks_y, chunks_z]"""
    nx, ny, nz = cells.shape[:3]
    m = cells[..., 0] != 0
    return m.reshape(nx // S, S, ny // S, S, nz // S, S).any(axis=(1, 3, 5))


TAGS = ("broadleaf", "conifer", "cross_x", "cross_z", "cross_y", "overlap", "edge_clip", "top_clip", "cactus", "rock_neighbour", "beach35", "lake", "ocean",
        "slope_edge", "air_chunk", "no_leaves")


def canopy_box(t):
    gx, gz, conifer, base, th, r = t[:6]
    cbase = base + th - (2 if conifer else 1)
    return gx - r, gx + r, gz - r, gz + r, cbase - (0 if conifer else 1), cbase + 2


def window_tags(cfg, cells, f, placed, ox=0, oz=0):
    """What a window shows, from generate_world's own output (tests/test_worldpregen_cpu.py asserts the chosen windows' union;
    profiles/worldpregen_windows.py searches with it)."""
    S = cfg.size
    nx, ny, nz = cells.shape[:3]
    out = set()
    trees = placed["trees"]
    for t in trees:
        out.add("conifer" if t[2] else "broadleaf")
        x0, x1, z0, z1, y0, y1 = canopy_box(t)
        if x0 < 0 or x1 >= nx or z0 < 0 or z1 >= nz:
            out.add("edge_clip")
        if max(x0, 0) // S != min(x1, nx - 1) // S:
            out.add("cross_x")
        if max(z0, 0) // S != min(z1, nz - 1) // S:
            out.add("cross_z")
        if max(y0, 0) // S != min(y1, ny - 1) // S:
            out.add("cross_y")
        if t[6]:
            out.add("top_clip")
        if not t[7]:
            out.add("no_leaves")
    for i, a in enumerate(trees):
        for b in trees[i + 1:]:
            A, B = canopy_box(a), canopy_box(b)
            if A[0] <= B[1] and B[0] <= A[1] and A[2] <= B[3] and B[2] <= A[3] and A[4] <= B[5] and B[4] <= A[5]:
                out.add("overlap")
    if placed["cacti"]:
        out.add("cactus")
    for gx, gz in placed["rocks"]:
        y = int(f["ground"][gx, gz]) + 1
        for x2, z2 in ((gx - 1, gz), (gx + 1, gz), (gx, gz - 1), (gx, gz + 1)):
            if 0 <= x2 < nx and 0 <= z2 < nz and y < ny and tuple(cells[x2, y, z2]) == (R.STONE, 1):
                out.add("rock_neighbour")
    d = f["water"] - f["ground"]
    if ((f["water"] > cfg.sea) & (d == 3)).any():
        out.add("beach35")
    if (f["biome"] == R.LAKES).any():
        out.add("lake")
    if (f["biome"] == R.OCEAN).any():
        out.add("ocean")
    wide = noise_fields(cfg, nx + 2, nz + 2, ox - 1, oz - 1)["ground0"]          # (nothing is ever carved: the ground is HeightY)
    dx = (wide[2:, 1:-1] - wide[:-2, 1:-1]).astype(F) * F(0.5)
    dz = (wide[1:-1, 2:] - wide[1:-1, :-2]).astype(F) * F(0.5)
    free = R.saturate(np.sqrt(dx * dx + dz * dz) / F(6))
    if (free != f["slope"]).any():
        out.add("slope_edge")
    if not chunk_occupied(cells, S).all():
        out.add("air_chunk")
    return out
