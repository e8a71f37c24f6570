"""An independent numpy-float32 restatement of WorldGenerator.GenerateChunkCells (reference Scenes/WorldGeneration/*.cs), written from the
C# and not from csrc/ycge_worldgen.h: what tests/test_worldgen_cpu.py holds the host export to.

Every fp32 operation is one numpy float32 operation (numpy does not fuse); arrays are the (S + 2)^2 tile of a chunk column or its S^2
interior.  MathF.Pow is csrc/ycge_math.h's m_pow restated in Python floats (IEEE binary64, no fusion).  Trees are placed by a plain
serial loop.  The river step is the literal ascending sort (river_accum_sorted); river_accum_indegree is the closed form the library uses.
"""
import math
import struct

import numpy as np

F = np.float32
AIR, STONE, DIRT, GRASS, WATER, SAND, WOOD, LEAVES, SNOW, TALLGRASS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 10
OCEAN, BEACH, LAKES, PLAINS, FOREST, DESERT, TAIGA, ALPINE = range(8)
ISLAND_RADIUS = F(10000.0)
INV_SQRT2, PERLIN2D = F(0.70710678118), F(1.41421356237)


class Config:          # WorldConfig.cs:19-34
    def __init__(self, chunk_size, chunks_y, seed):
        self.size, self.seed = chunk_size, seed
        self.height = chunks_y * chunk_size
        self.sea = max(1, self.height // 4)
        self.snow = int(F(self.height) * F(0.8))


def fast_hash(x, y, z, seed):          # GenMath.cs:165-175; x, z int64 arrays
    M = np.uint64(0xFFFFFFFF)
    h = np.uint64((2166136261 ^ (seed & 0xFFFFFFFF)) & 0xFFFFFFFF)
    P = np.uint64(16777619)
    h = ((h ^ (np.asarray(x).astype(np.int64).astype(np.uint64) & M)) * P) & M
    h = ((h ^ np.uint64(y & 0xFFFFFFFF)) * P) & M
    h = ((h ^ (np.asarray(z).astype(np.int64).astype(np.uint64) & M)) * P) & M
    return h.astype(np.uint32)


def fast_floor(t):          # :108
    i = np.trunc(t).astype(np.int64)
    return np.where(t >= F(0), i, i - 1)


def fade(t):          # :110
    return t * t * t * (t * (t * F(6) - F(15)) + F(10))


def lerp(a, b, t):
    return a + (b - a) * t


def saturate(x):
    return np.where(x < F(0), F(0), np.where(x > F(1), F(1), x)).astype(F)


def grad_dot(ix, iz, seed, x, z):          # :112-126, :152
    k = (fast_hash(ix, 0, iz, seed) >> np.uint32(13)) & np.uint32(7)
    g0 = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6], [F(1), F(-1), F(0), F(0), INV_SQRT2, -INV_SQRT2, INV_SQRT2], -INV_SQRT2).astype(F)
    g1 = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5, k == 6], [F(0), F(0), F(1), F(-1), INV_SQRT2, INV_SQRT2, -INV_SQRT2], -INV_SQRT2).astype(F)
    return g0 * x + g1 * z


def gradient_noise2(x, z, seed):          # :52-70
    x, z = np.asarray(x, F), np.asarray(z, F)
    x0, z0 = fast_floor(x), fast_floor(z)
    tx, tz = x - x0.astype(F), z - z0.astype(F)
    u, v = fade(tx), fade(tz)
    n00 = grad_dot(x0, z0, seed, tx, tz)
    n10 = grad_dot(x0 + 1, z0, seed, tx - F(1), tz)
    n01 = grad_dot(x0, z0 + 1, seed, tx, tz - F(1))
    n11 = grad_dot(x0 + 1, z0 + 1, seed, tx - F(1), tz - F(1))
    val = lerp(lerp(n00, n10, u), lerp(n01, n11, u), v) * PERLIN2D
    return np.where(val < F(-1), F(-1), np.where(val > F(1), F(1), val)).astype(F)


def fbm2(x, z, octaves, seed):          # :8-19 with lacunarity 2, gain 0.5, baseFreq 1 (every call site)
    s, amp, freq = np.zeros_like(np.asarray(x, F)), F(1), F(1)
    for i in range(octaves):
        s = s + gradient_noise2(x * freq, z * freq, seed + i * 131) * amp
        freq, amp = freq * F(2), amp * F(0.5)
    return F(0.5) * s + F(0.5)


def ridged2(x, z, octaves, seed):          # :21-37
    s, amp, freq, weight = np.zeros_like(np.asarray(x, F)), F(0.5), F(1), np.ones_like(np.asarray(x, F))
    for i in range(octaves):
        n = gradient_noise2(x * freq, z * freq, seed + i * 733)
        n = F(1) - np.abs(n)
        n = n * n
        n = n * weight
        weight = n * F(0.5)
        weight = np.where(weight > F(1), F(1), weight).astype(F)
        s = s + n * amp
        freq, amp = freq * F(2), amp * F(0.5)
    return s


# ---- m_pow (csrc/ycge_math.h) in binary64
def _bits(d): return struct.unpack("<Q", struct.pack("<d", d))[0]
def _dbl(b): return struct.unpack("<d", struct.pack("<Q", b))[0]


def m_log_d(x):
    b = _bits(x)
    e = ((b >> 52) & 0x7ff) - 1023
    m = _dbl((b & 0x000fffffffffffff) | 0x3ff0000000000000)
    if m > 1.41421356237309514547:
        m, e = m * 0.5, e + 1
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    p = 1.0 / 23.0
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * s2 + 1.0 / d
    p = p * s2 + 1.0
    de = float(e)
    return (de * 6.93147180369123816490e-01 + (2.0 * s) * p) + de * 1.90821492927058770002e-10


def m_exp_d(x):
    kf = x * 1.44269504088896338700e+00
    k = int(kf - 0.5 if kf < 0.0 else kf + 0.5)
    dk = float(k)
    r = (x - dk * 6.93147180369123816490e-01) - dk * 1.90821492927058770002e-10
    r2 = r * r; r4 = r2 * r2; r8 = r4 * r4
    a0 = 1.0 + 1.0 * r
    a1 = 5.0000000000000000000e-01 + 1.6666666666666666667e-01 * r
    a2 = 4.1666666666666666667e-02 + 8.3333333333333333333e-03 * r
    a3 = 1.3888888888888888889e-03 + 1.9841269841269841270e-04 * r
    a4 = 2.4801587301587301587e-05 + 2.7557319223985890653e-06 * r
    a5 = 2.7557319223985890653e-07 + 2.5052108385441718775e-08 * r
    a6 = 2.0876756987868098979e-09 + 1.6059043836821614599e-10 * r
    q0, q1, q2 = a0 + a1 * r2, a2 + a3 * r2, a4 + a5 * r2
    h0, h1 = q0 + q1 * r4, q2 + a6 * r4
    return math.ldexp(h0 + h1 * r8, k)


def m_pow(x, y):
    out = np.empty_like(x)
    for i, v in np.ndenumerate(x):
        out[i] = F(0) if v == 0 else F(1) if v == 1 else F(m_exp_d(float(F(y)) * m_log_d(float(v))))
    return out


# ---- TerrainNoise.cs
def warp(x, z, seed):          # :21-35
    wx1 = fbm2(x * F(0.00025), z * F(0.00025), 4, seed + 101)
    wz1 = fbm2((x + F(137)) * F(0.00025), (z - F(271)) * F(0.00025), 4, seed + 103)
    x = x + (wx1 - F(0.5)) * F(2) * F(350)
    z = z + (wz1 - F(0.5)) * F(2) * F(350)
    wx2 = fbm2(x * F(0.0012), z * F(0.0012), 3, seed + 151)
    wz2 = fbm2((x - F(911)) * F(0.0012), (z + F(643)) * F(0.0012), 3, seed + 157)
    x = x + (wx2 - F(0.5)) * F(2) * F(90)
    z = z + (wz2 - F(0.5)) * F(2) * F(90)
    return x, z


def shore(x, z, seed):          # :13-18 / :44-49
    dist = np.sqrt(x * x + z * z)
    jit = (fbm2(x * F(0.00022), z * F(0.00022), 3, seed + 333) - F(0.5)) * F(2) * F(600)
    dist = np.maximum(F(0), dist - jit)
    fade_w = max(F(8), ISLAND_RADIUS * F(0.18))
    e0 = ISLAND_RADIUS - fade_w
    t = saturate((dist - e0) / (ISLAND_RADIUS - e0))
    return F(1) - t * t * (F(3) - F(2) * t)


def height_y(gx, gz, cfg):          # :38-110; gx, gz int arrays
    x, z = warp(gx.astype(F), gz.astype(F), cfg.seed)
    mask = shore(x, z, cfg.seed)
    n_cont = ridged2(x * F(0.00045), z * F(0.00045), 6, cfg.seed + 1001)
    n_mount = ridged2(x * F(0.0011), z * F(0.0011), 5, cfg.seed + 1003)
    d1 = fbm2(x * F(0.0025), z * F(0.0025), 6, cfg.seed + 1005)
    d2 = fbm2(x * F(0.0060), z * F(0.0060), 5, cfg.seed + 1006)
    mmask = saturate((n_cont * F(1.15) + n_mount * F(1.10)) - F(0.90))
    plains = d1 * F(0.65) + d2 * F(0.35)
    h01 = lerp(plains, m_pow(n_mount, 1.35), mmask)
    cf = saturate(np.sqrt(x * x + z * z) / (ISLAND_RADIUS * F(0.55)))
    h01 = h01 * lerp(F(0.55), F(1.0), cf)
    h01 = saturate(np.minimum(h01, mask))
    max_rise = F(cfg.height) * F(0.45)
    h = np.rint(F(cfg.sea) + h01 * max_rise).astype(np.int64)
    ocean_floor = max(1, cfg.sea - 12)
    fx, fz = gx.astype(F), gz.astype(F)
    radial = saturate(F(1) - np.sqrt(fx * fx + fz * fz) / ISLAND_RADIUS)
    bed = fbm2(fx * F(0.0015), fz * F(0.0015), 3, cfg.seed + 1303)
    und = np.rint((bed - F(0.5)) * F(6)).astype(np.int64)
    h = np.where(radial <= F(0.0005), ocean_floor + und, np.maximum(h, ocean_floor))
    return np.clip(h, 0, cfg.height - 1)


def local_water_y(gx, gz, cfg, ground, slope):          # :113-136
    x, z = warp(gx.astype(F), gz.astype(F), cfg.seed)
    mask = shore(x, z, cfg.seed)
    fx, fz = gx.astype(F), gz.astype(F)
    n1 = fbm2(fx * F(0.0008), fz * F(0.0008), 5, cfg.seed + 8101)
    n2 = fbm2(fx * F(0.0016), fz * F(0.0016), 4, cfg.seed + 8107)
    lake = F(0.65) * n1 + F(0.35) * n2
    low = saturate(F(1) - (ground - cfg.sea).astype(F) / max(F(1), F(cfg.snow - cfg.sea)))
    cand = F(cfg.sea) + F(8) + (lake * F(0.75) + low * F(0.25)) * F(60)
    wy = np.floor(cand).astype(np.int64)
    ok = (mask >= F(0.05)) & (slope <= F(0.60)) & (ground.astype(F) + F(1) < cand) & (wy > cfg.sea)
    return np.where(ok, wy, cfg.sea)


# ---- RiverNetwork.cs
def d8(tile, S):          # :31-56 -> (dnX, dnZ)
    dnx, dnz = np.zeros((S, S), np.int64), np.zeros((S, S), np.int64)
    best = np.zeros((S, S), np.int64)
    h0 = tile[1:S + 1, 1:S + 1]
    for oz in (-1, 0, 1):
        for ox in (-1, 0, 1):
            if ox == 0 and oz == 0:
                continue
            drop = h0 - tile[1 + ox:S + 1 + ox, 1 + oz:S + 1 + oz]
            better = drop > best
            best = np.where(better, drop, best); dnx = np.where(better, ox, dnx); dnz = np.where(better, oz, dnz)
    return dnx, dnz


def river_accum_sorted(ground, dnx, dnz):          # :58-78, literally (a stable ascending sort; ties in index order)
    S = ground.shape[0]
    order = sorted(((int(ground[x, z]), x, z) for x in range(S) for z in range(S)), key=lambda c: c[0])
    accum = np.zeros((S, S), F)
    for _, x, z in order:
        a = accum[x, z]
        if a <= 0:
            a = F(1)
        nx, nz = x + int(dnx[x, z]), z + int(dnz[x, z])
        if 0 <= nx < S and 0 <= nz < S:
            accum[nx, nz] += a
    return accum


def river_accum_indegree(dnx, dnz):          # what the sort comes to: in-chunk neighbours draining here, plus 1 for a cell with no lower neighbour (it "drains" into itself)
    S = dnx.shape[0]
    accum = np.zeros((S, S), F)
    for x in range(S):
        for z in range(S):
            nx, nz = x + int(dnx[x, z]), z + int(dnz[x, z])
            if 0 <= nx < S and 0 <= nz < S:
                accum[nx, nz] += F(1)
    return accum


def carve_and_surface(accum, ground, sea):
    """RiverNetwork.cs:80-113: (carved ground, river surface) from the accumulation."""
    accum = np.asarray(accum, F)
    t = (accum - F(50)) / F(50)
    carve = np.where(t <= 0, F(0), np.minimum(F(3.5), np.maximum(F(0), t) * F(3.5))).astype(F)
    river_water = np.where(t <= 0, sea, np.maximum(sea, ground - np.floor(carve).astype(np.int64) + int(math.ceil(2.0))))
    lower = np.floor(carve).astype(np.int64)
    return np.where(lower > 0, np.maximum(0, ground - lower), ground), river_water


def columns(cx, cz, cfg, accum_fn=None):
    """WorldGenerator.cs:104-154: ground (carved), localWater, biome, slope01 over the chunk column, and the uncarved tile."""
    S = cfg.size
    lx, lz = np.meshgrid(np.arange(-1, S + 1), np.arange(-1, S + 1), indexing="ij")
    tile = height_y(cx * S + lx, cz * S + lz, cfg)
    ground = tile[1:S + 1, 1:S + 1].copy()
    dnx, dnz = d8(tile, S)
    accum = river_accum_sorted(ground, dnx, dnz) if accum_fn is None else accum_fn(dnx, dnz)
    ground, river_water = carve_and_surface(accum, ground, cfg.sea)
    idx = np.arange(S)
    a, b = np.maximum(0, idx - 1), np.minimum(S - 1, idx + 1)
    dx = (ground[b, :] - ground[a, :]).astype(F) * F(0.5)
    dz = (ground[:, b] - ground[:, a]).astype(F) * F(0.5)
    slope = saturate(np.sqrt(dx * dx + dz * dz) / F(6))
    gx, gz = cx * S + lx[1:S + 1, 1:S + 1], cz * S + lz[1:S + 1, 1:S + 1]
    fx, fz = gx.astype(F), gz.astype(F)
    m1 = fbm2(fx * F(0.0025), fz * F(0.0025), 5, cfg.seed + 5002)
    r1 = ridged2(fx * F(0.0020), fz * F(0.0020), 4, cfg.seed + 5003)
    dry = F(0.55) * r1 + F(0.45) * (F(1) - m1)
    biome = np.where(ground <= cfg.sea - 1, OCEAN, np.where(np.abs(ground - cfg.sea) <= 2, BEACH, np.where(dry > F(0.52), DESERT, FOREST)))
    water = np.maximum(local_water_y(gx, gz, cfg, ground, slope), river_water)
    biome = np.where((water > cfg.sea) & (ground <= water), LAKES, biome)
    rock_n = fbm2(fx * F(0.004), fz * F(0.004), 3, cfg.seed + 4201)
    return dict(ground=ground, water=water, biome=biome, slope=slope, rock_n=rock_n, tile=tile, gx=gx, gz=gz)


def flora_hash(x, z, seed):          # FloraPlacer.cs:7-16
    h = int(fast_hash(np.int64(x), 0, np.int64(z), seed))
    h ^= (h << 13) & 0xFFFFFFFF; h ^= h >> 17; h ^= (h << 5) & 0xFFFFFFFF
    return h


def trees(col, cy, cfg):
    """FloraPlacer.cs:27-69: [(lx, lz, conifer, trunkBase, trunkH (after shortening), canopyR, desiredTop)] in (lx, lz) order."""
    S, out = cfg.size, []
    for lx in range(S):
        for lz in range(S):
            gY, wY = int(col["ground"][lx, lz]), int(col["water"][lx, lz])
            top = gY - cy * S
            if top < 0 or top >= S or gY <= wY or gY >= cfg.snow - 2 or col["slope"][lx, lz] > F(0.45) or col["biome"][lx, lz] != FOREST:
                continue
            h = flora_hash(int(col["gx"][lx, lz]), int(col["gz"][lx, lz]), cfg.seed + 90001)
            if F(h & 0xFFFF) / F(65535.0) > F(0.03):
                continue
            conifer = ((h >> 16) & 3) == 0
            base = top + 1
            th = 6 + ((h >> 2) & 7) if conifer else 4 + ((h >> 3) & 5)
            r = 2 if conifer else 2 + ((h >> 6) & 1)
            desired = base + th - (2 if conifer else 1) + 2
            if desired > S - 1:
                th = max(3, th - (desired - (S - 1)))
            out.append((lx, lz, conifer, base, th, r, desired))
    return out


def generate_chunk(cx, cy, cz, cfg, col=None):
    """-> (cells int32 [S, S, S, 2] in (lx, ly, lz) order, any_solid)"""
    S = cfg.size
    col = columns(cx, cz, cfg) if col is None else col
    cells = np.zeros((S, S, S, 2), np.int32)
    gy = cy * S + np.arange(S)[None, :, None]
    gY, wY = col["ground"][:, None, :], col["water"][:, None, :]
    biome, slope = col["biome"][:, None, :], col["slope"][:, None, :]
    surface = np.where(gY >= cfg.snow, SNOW, np.where(np.abs(gY - cfg.sea) <= 2, SAND, np.where(slope > F(0.80), STONE, np.where(biome == DESERT, SAND, GRASS))))
    surface = np.where((wY > cfg.sea) & (wY - gY <= 2), SAND, surface)
    sub = np.where(gY <= cfg.sea + 1, SAND, np.where(biome == DESERT, SAND, np.where(gY - gy <= 3, DIRT, STONE)))
    mat = np.where(gy > gY, np.where(gy <= wY, WATER, AIR), np.where(gy == gY, surface, np.where(gy >= gY - 3, sub, STONE)))
    band = (np.fmod(gy, 24)).astype(F) / F(24)
    base_meta = np.where(band < F(0.33), 0, np.where(band < F(0.66), 1, 2))
    n = col["rock_n"][:, None, :]
    meta = np.where(n < F(0.33), 0, np.where(n < F(0.66), 1, base_meta))
    cells[..., 0] = mat
    cells[..., 1] = np.where((gy < gY - 3), meta, 0)
    for lx, lz, conifer, base, th, r, _ in trees(col, cy, cfg):          # :71-131
        for t in range(th):
            ly = base + t
            if 0 <= ly < S and cells[lx, ly, lz, 0] in (AIR, TALLGRASS):
                cells[lx, ly, lz] = (WOOD, 0)
        cbase, any_leaves = base + th - (2 if conifer else 1), False
        for dy in range(0 if conifer else -1, 3):
            ly = cbase + dy
            if not 0 <= ly < S:
                continue
            rad = max(1, r - abs(dy)) if conifer else r - (1 if dy == 2 else 0)
            for rx in range(-rad, rad + 1):
                for rz in range(-rad, rad + 1):
                    x2, z2 = lx + rx, lz + rz
                    if 0 <= x2 < S and 0 <= z2 < S and cells[x2, ly, z2, 0] in (AIR, TALLGRASS):
                        cells[x2, ly, z2] = (LEAVES, 0); any_leaves = True
        if not any_leaves:
            ly = base + th - 1
            if 0 <= ly < S:
                for rx in (-1, 0, 1):
                    for rz in (-1, 0, 1):
                        x2, z2 = lx + rx, lz + rz
                        if 0 <= x2 < S and 0 <= z2 < S and cells[x2, ly, z2, 0] == AIR:
                            cells[x2, ly, z2] = (LEAVES, 0)
    return cells, bool((cells[..., 0] != 0).any())
