// ycge_worldgen.h - WorldGenerator.GenerateChunkCells restated for host and gfx950 (Scenes/WorldGeneration/*.cs of the reference).
//
// One chunk of the voxel world is a pure function of (cx, cy, cz, WorldConfig): integer hashing and fp32 + - * / sqrt floor round, plus
// one MathF.Pow.  Everything here obeys ycge_math.h's contract (no contraction, correctly rounded divide and sqrt, m_pow for the power), so
// the host generator (ycge_worldgen.cpp) and the kernels (ycge_worldgen.hip) give the same cells, bit for bit.
//
// IslandSettings (IslandSettings.cs:5-54) and the WorldGenSettings fields the generator reads (WorldGenSettings.cs) are compile-time
// constants at the reference's values.  Not restated: the whole-world pregen path (RiverNetworkGlobal, PlaceTreesGlobal), the dead
// FBM3D / GradientNoise3D / GetBlockAt, SimpleEntityPlacer.
//
// The work is cut where the data flow cuts it:
//   height_y            TerrainNoise.HeightY: once per cell of the (S + 2)^2 tile around a chunk column (cx, cz)
//   d8_direction        RiverNetwork.cs:31-56, from the tile
//   river_accum         RiverNetwork.cs:58-78 (see there: an in-degree count)
//   river_carve         RiverNetwork.cs:80-113
//   column_record       WorldGenerator.cs:125-154 + StrataMap's noise verdict: what every cy of the column shares
//   cell_at             WorldGenerator.cs:156-199, one cell from its column's record
//   tree_at + the tree_* helpers   FloraPlacer.cs:27-69; the placement loops (:71-131) are the callers'
#pragma once
#include "ycge_math.h"

namespace ycge {
namespace wg {

// ---- IslandSettings.cs
constexpr float kIslandRadius = 10000.0f, kMaskFadeFraction = 0.18f, kMaxRiseFraction = 0.45f;
constexpr int kSeaFloorDepth = 12, kBeachBuffer = 2, kIslandDirtDepth = 3;
constexpr float kCoastJitterFreq = 0.00022f, kCoastJitterAmp = 600.0f;
constexpr float kWarp1Freq = 0.00025f, kWarp1Amp = 350.0f, kWarp2Freq = 0.0012f, kWarp2Amp = 90.0f;
constexpr float kContinentFreq = 0.00045f, kMountainFreq = 0.0011f, kDetail1Freq = 0.0025f, kDetail2Freq = 0.0060f;
constexpr int kContinentOctaves = 6, kMountainOctaves = 5, kDetail1Octaves = 6, kDetail2Octaves = 5;
constexpr float kLakeFreq1 = 0.0008f, kLakeFreq2 = 0.0016f, kLakeRiseMax = 60.0f, kLakeBaseAboveSea = 8.0f, kLakeSlopeMax = 0.60f;
constexpr float kLakeMaskThreshold = 0.05f, kLakeMinDepth = 1.0f;
constexpr float kTerraceStep = 0.0f, kTerraceJitter = 0.15f;
constexpr float kRiverAccumThreshold = 50.0f, kRiverMaxCarve = 3.5f, kRiverWaterDepth = 2.0f;
// ---- WorldGenSettings.cs
constexpr int kAir = 0, kStone = 1, kDirt = 2, kGrass = 3, kWater = 4, kSand = 5, kWood = 6, kLeaves = 7, kSnow = 8, kTallGrass = 10;   // Blocks, :8-22
constexpr int kTerrainDirtDepth = 3, kUnderwaterSandBuffer = 1;                                                                     // Terrain, :32-39
constexpr float kInvSqrt2 = 0.70710678118f, kPerlin2D = 1.41421356237f, kSlopeNormalize = 6.0f;                                      // Normalization, :157-164
constexpr uint32_t kFnvOffset = 2166136261u, kFnvPrime = 16777619u;                                                                 // Hashing, :166-170
// ---- Biome.cs
enum Biome : int { kOcean = 0, kBeach, kLakes, kPlains, kForest, kDesert, kTaiga, kAlpine, kSnowBiome };

// WorldConfig (WorldConfig.cs:19-34), the fields the generator reads
struct World {
    int size;            // ChunkSize
    int height;          // WorldHeight = ChunksY * ChunkSize
    int seed;            // WorldSeed
    int sea, snow;       // WaterLevel, SnowLevel
};
YCGE_HD World make_world(int chunk_size, int chunks_y, int seed)
{
    World W;
    W.size = chunk_size; W.height = chunks_y * chunk_size; W.seed = seed;
    W.sea = W.height / 4 > 1 ? W.height / 4 : 1;          // Math.Max(1, WorldHeight / 4), :32
    W.snow = cs_f2i((float)W.height * 0.8f);             // (int)(WorldHeight * 0.8f), :33
    return W;
}

// what all cy of one (lx, lz) column share
struct ColRec {
    int32_t ground;      // carved
    int32_t water;       // localWater
    float slope;
    int32_t biome_rock;  // biome | rock verdict << 8 (0: meta 0, 1: meta 1, 2: the altitude band's meta - StrataMap.cs:15-18)
};

// ---------------------------------------------------------------------------------------------------------------- GenMath.cs
YCGE_HD uint32_t fast_hash(int x, int y, int z, int seed)          // :165-175
{
    uint32_t h = kFnvOffset ^ (uint32_t)seed;
    h ^= (uint32_t)x; h *= kFnvPrime;
    h ^= (uint32_t)y; h *= kFnvPrime;
    h ^= (uint32_t)z; h *= kFnvPrime;
    return h;
}
YCGE_HD int fast_floor(float t) { return t >= 0.0f ? cs_f2i(t) : cs_f2i(t) - 1; }          // :108
YCGE_HD float fade(float t) { return t * t * t * (t * (t * 6.0f - 15.0f) + 10.0f); }        // :110
YCGE_HD float lerp(float a, float b, float t) { return a + (b - a) * t; }                   // :154
YCGE_HD float smooth_step(float e0, float e1, float x)                                      // :159-163
{
    const float t = clamp01((x - e0) / (e1 - e0));
    return t * t * (3.0f - 2.0f * t);
}
// Dot(Grad2(ix, iz, seed), x, z), :112-126, :152 - the switch over new float[] { .. } as selects on (h >> 13) & 7
YCGE_HD float grad_dot(int ix, int iz, int seed, float x, float z)
{
    const uint32_t k = (fast_hash(ix, 0, iz, seed) >> 13) & 7u;
    const float d = (k & 1u) ? -kInvSqrt2 : kInvSqrt2, e = (k & 2u) ? -kInvSqrt2 : kInvSqrt2;
    const float g0 = k >= 4u ? d : (k == 0u ? 1.0f : (k == 1u ? -1.0f : 0.0f));
    const float g1 = k >= 4u ? e : (k == 2u ? 1.0f : (k == 3u ? -1.0f : 0.0f));
    return g0 * x + g1 * z;
}
YCGE_HD float gradient_noise2(float x, float z, int seed)          // :52-70
{
    const int x0 = fast_floor(x), z0 = fast_floor(z);
    const int x1 = x0 + 1, z1 = z0 + 1;
    const float tx = x - (float)x0, tz = z - (float)z0;
    const float u = fade(tx), v = fade(tz);
    const float n00 = grad_dot(x0, z0, seed, tx, tz);
    const float n10 = grad_dot(x1, z0, seed, tx - 1.0f, tz);
    const float n01 = grad_dot(x0, z1, seed, tx, tz - 1.0f);
    const float n11 = grad_dot(x1, z1, seed, tx - 1.0f, tz - 1.0f);
    const float ix0 = lerp(n00, n10, u), ix1 = lerp(n01, n11, u);
    return cs_clamp(lerp(ix0, ix1, v) * kPerlin2D, -1.0f, 1.0f);
}
// every call site passes lacunarity 2, gain 0.5, baseFreq 1 (kept as arguments: the products are the reference's)
YCGE_HD float fbm2(float x, float z, int octaves, float lacunarity, float gain, float base_freq, int seed)          // :8-19
{
    float sum = 0.0f, amp = 1.0f, freq = base_freq;
#pragma unroll 1
    for (int i = 0; i < octaves; i++) {
        const float n = gradient_noise2(x * freq, z * freq, seed + i * 131);
        sum += n * amp;
        freq *= lacunarity;
        amp *= gain;
    }
    return 0.5f * sum + 0.5f;
}
YCGE_HD float ridged_fbm2(float x, float z, int octaves, float lacunarity, float gain, float base_freq, int seed)   // :21-37
{
    float sum = 0.0f, amp = 0.5f, freq = base_freq, weight = 1.0f;
#pragma unroll 1
    for (int i = 0; i < octaves; i++) {
        float n = gradient_noise2(x * freq, z * freq, seed + i * 733);
        n = 1.0f - cs_abs(n);
        n *= n;
        n *= weight;
        weight = n * gain;
        if (weight > 1.0f) weight = 1.0f;
        sum += n * amp;
        freq *= lacunarity;
        amp *= 0.5f;
    }
    return sum;
}

// ---------------------------------------------------------------------------------------------------------------- TerrainNoise.cs
YCGE_HD void warp(float &x, float &z, int seed)          // :21-35
{
    float wx1 = fbm2(x * kWarp1Freq, z * kWarp1Freq, 4, 2.0f, 0.5f, 1.0f, seed + 101);
    float wz1 = fbm2((x + 137.0f) * kWarp1Freq, (z - 271.0f) * kWarp1Freq, 4, 2.0f, 0.5f, 1.0f, seed + 103);
    wx1 = (wx1 - 0.5f) * 2.0f; wz1 = (wz1 - 0.5f) * 2.0f;
    x += wx1 * kWarp1Amp;
    z += wz1 * kWarp1Amp;
    float wx2 = fbm2(x * kWarp2Freq, z * kWarp2Freq, 3, 2.0f, 0.5f, 1.0f, seed + 151);
    float wz2 = fbm2((x - 911.0f) * kWarp2Freq, (z + 643.0f) * kWarp2Freq, 3, 2.0f, 0.5f, 1.0f, seed + 157);
    wx2 = (wx2 - 0.5f) * 2.0f; wz2 = (wz2 - 0.5f) * 2.0f;
    x += wx2 * kWarp2Amp;
    z += wz2 * kWarp2Amp;
}
// the shoreline mask of the WARPED point, :13-18 = :44-49
YCGE_HD float shore_mask(float x, float z, int seed)
{
    float dist = cs_sqrt(x * x + z * z);
    const float coast_jitter = (fbm2(x * kCoastJitterFreq, z * kCoastJitterFreq, 3, 2.0f, 0.5f, 1.0f, seed + 333) - 0.5f) * 2.0f * kCoastJitterAmp;
    dist = cs_max(0.0f, dist - coast_jitter);
    const float fade_w = cs_max(8.0f, kIslandRadius * kMaskFadeFraction);
    const float edge_start = kIslandRadius - fade_w;
    return 1.0f - smooth_step(edge_start, kIslandRadius, dist);
}
YCGE_HD float island_mask01(float gx, float gz, const World &W)          // :9-19
{
    float x = gx, z = gz;
    warp(x, z, W.seed);
    return shore_mask(x, z, W.seed);
}
YCGE_HD float height01(float gx, float gz, const World &W)               // :38-83
{
    float x = gx, z = gz;
    warp(x, z, W.seed);
    const float mask = shore_mask(x, z, W.seed);
    const int seed = W.seed;
    const float n_cont = ridged_fbm2(x * kContinentFreq, z * kContinentFreq, kContinentOctaves, 2.0f, 0.5f, 1.0f, seed + 1001);
    const float n_mount = ridged_fbm2(x * kMountainFreq, z * kMountainFreq, kMountainOctaves, 2.0f, 0.5f, 1.0f, seed + 1003);
    const float d1 = fbm2(x * kDetail1Freq, z * kDetail1Freq, kDetail1Octaves, 2.0f, 0.5f, 1.0f, seed + 1005);
    const float d2 = fbm2(x * kDetail2Freq, z * kDetail2Freq, kDetail2Octaves, 2.0f, 0.5f, 1.0f, seed + 1006);
    const float mountain_mask = clamp01((n_cont * 1.15f + n_mount * 1.10f) - 0.90f);
    const float plains = d1 * 0.65f + d2 * 0.35f;
    const float mountains = m_pow(n_mount, 1.35f);          // MathF.Pow
    const float base_terrain = lerp(plains, mountains, mountain_mask);
    float h01 = base_terrain;
    const float center_dist = cs_sqrt(x * x + z * z);
    const float center_flatten = clamp01(center_dist / (kIslandRadius * 0.55f));
    h01 *= lerp(0.55f, 1.00f, center_flatten);
    if (kTerraceStep > 0.0f) {          // :72-78 as written; TerraceStep is 0
        const float step = kTerraceStep / cs_max(1.0f, (float)W.height);
        const float terr_jitter = (fbm2(x * 0.01f, z * 0.01f, 2, 2.0f, 0.5f, 1.0f, seed + 707) - 0.5f) * 2.0f * kTerraceJitter * step;
        const float q = cs_floor((h01 + terr_jitter) / step) * step;
        h01 = clamp01(q);
    }
    h01 = cs_min(h01, mask);
    return clamp01(h01);
}
// MathF.Round: to nearest, ties to even (v_rndne_f32 / the host's default rounding mode)
YCGE_HD float round_even(float f) { return __builtin_rintf(f); }
YCGE_HD int height_y(int gx, int gz, const World &W)                    // :85-110
{
    const int sea = W.sea;
    const int ocean_floor = sea - kSeaFloorDepth > 1 ? sea - kSeaFloorDepth : 1;
    const float h01 = height01((float)gx, (float)gz, W);
    const float max_rise = (float)W.height * kMaxRiseFraction;
    int h = cs_f2i(round_even((float)sea + h01 * max_rise));
    const float dx = (float)gx, dz = (float)gz;
    const float radial = clamp01(1.0f - cs_sqrt(dx * dx + dz * dz) / kIslandRadius);
    if (radial <= 0.0005f) {
        const float bed = fbm2((float)gx * 0.0015f, (float)gz * 0.0015f, 3, 2.0f, 0.5f, 1.0f, W.seed + 1303);
        const int undulate = cs_f2i(round_even((bed - 0.5f) * 6.0f));
        h = ocean_floor + undulate;
    } else {
        h = h > ocean_floor ? h : ocean_floor;
    }
    if (h < 0) h = 0;
    if (h >= W.height) h = W.height - 1;
    return h;
}
YCGE_HD int local_water_y(int gx, int gz, const World &W, int ground_y, float slope01)          // :113-136
{
    const int sea = W.sea;
    const float mask = island_mask01((float)gx, (float)gz, W);
    if (mask < kLakeMaskThreshold) return sea;
    const int seed = W.seed;
    const float n1 = fbm2((float)gx * kLakeFreq1, (float)gz * kLakeFreq1, 5, 2.0f, 0.5f, 1.0f, seed + 8101);
    const float n2 = fbm2((float)gx * kLakeFreq2, (float)gz * kLakeFreq2, 4, 2.0f, 0.5f, 1.0f, seed + 8107);
    const float lake_field = 0.65f * n1 + 0.35f * n2;
    const float lowland_bias = clamp01(1.0f - (float)(ground_y - sea) / cs_max(1.0f, (float)(W.snow - sea)));
    const float candidate = (float)sea + kLakeBaseAboveSea + (lake_field * 0.75f + lowland_bias * 0.25f) * kLakeRiseMax;
    if (slope01 <= kLakeSlopeMax && (float)ground_y + kLakeMinDepth < candidate) {
        const int wy = cs_f2i(cs_floor(candidate));
        if (wy > sea) return wy;
    }
    return sea;
}

// ---------------------------------------------------------------------------------------------------------------- RiverNetwork.cs
// `tile`: HeightY over [-1, S] x [-1, S] of the chunk column, index (lx + 1) * (S + 2) + (lz + 1)
YCGE_HD int tile_at(const int *tile, int S, int lx, int lz) { return tile[(lx + 1) * (S + 2) + (lz + 1)]; }
// :31-56 - D8 steepest descent; the result is (dx + 1) * 3 + (dz + 1), 4 = no lower neighbour.  oz outer, ox inner, the first of equal drops wins.
YCGE_HD int d8_direction(const int *tile, int S, int lx, int lz)
{
    const int h0 = tile_at(tile, S, lx, lz);
    int best_dx = 0, best_dz = 0, best_drop = 0;
    for (int oz = -1; oz <= 1; oz++)
        for (int ox = -1; ox <= 1; ox++) {
            if (ox == 0 && oz == 0) continue;
            const int drop = h0 - tile_at(tile, S, lx + ox, lz + oz);
            if (drop > best_drop) { best_drop = drop; best_dx = ox; best_dz = oz; }
        }
    return (best_dx + 1) * 3 + (best_dz + 1);
}
// :58-78.  The reference sorts the chunk's cells by height ASCENDING and lets each, in that order, add max(accum, 1) to the cell it drains
// into.  A cell drains into a STRICTLY lower one, which the order has already passed: when a cell is processed nothing has reached it yet,
// so every cell adds exactly 1, and Array.Sort's order among equal heights cannot matter.  A cell with no lower neighbour has dn = (0, 0):
// it "drains" into itself and adds that 1 to its own total (:72-77 do not exclude it).  accum is therefore
//     (in-chunk neighbours whose D8 direction points here) + (1 if this cell has no lower neighbour)       <= 9
// `dir`: d8_direction over the chunk, index lx * S + lz.
YCGE_HD float river_accum(const uint8_t *dir, int S, int lx, int lz)
{
    int n = dir[lx * S + lz] == 4 ? 1 : 0;
    for (int ox = -1; ox <= 1; ox++)
        for (int oz = -1; oz <= 1; oz++) {
            if (ox == 0 && oz == 0) continue;
            const int nx = lx + ox, nz = lz + oz;
            if (nx < 0 || nx >= S || nz < 0 || nz >= S) continue;
            if (dir[nx * S + nz] == (1 - ox) * 3 + (1 - oz)) n++;          // its (dx, dz) = (-ox, -oz)
        }
    return (float)n;
}
// :80-113 - carve depth and river surface from the accumulation; returns the carved ground.  (With RiverAccumThreshold = 50 and
// accum <= 9, t <= 0 everywhere: nothing is carved and the river surface is the sea.  Restated in full all the same.)
YCGE_HD int river_carve(float accum, int ground, int sea, int *river_water)
{
    const float t = (accum - kRiverAccumThreshold) / kRiverAccumThreshold;
    if (t <= 0.0f) { *river_water = sea; return ground; }
    const float carve = cs_min(kRiverMaxCarve, cs_max(0.0f, t) * kRiverMaxCarve);
    const int bed_y = ground - cs_f2i(cs_floor(carve));
    const int surface = bed_y + cs_f2i(__builtin_ceilf(kRiverWaterDepth));
    *river_water = sea > surface ? sea : surface;
    const int lower = cs_f2i(cs_floor(carve));
    if (lower > 0) { const int g = ground - lower; return g > 0 ? g : 0; }
    return ground;
}

// ---------------------------------------------------------------------------------------------------------------- BiomeMap.cs, Layering.cs, StrataMap.cs
YCGE_HD int biome_evaluate(int gx, int gz, int height_y_, int sea, const World &W)          // BiomeMap.cs:7-22 (snow and slope01 are not read)
{
    if (height_y_ <= sea - 1) return kOcean;
    const int d = height_y_ - sea;
    if ((d < 0 ? -d : d) <= kBeachBuffer) return kBeach;
    const int seed = W.seed;
    const float m1 = fbm2((float)gx * 0.0025f, (float)gz * 0.0025f, 5, 2.0f, 0.5f, 1.0f, seed + 5002);
    const float d1 = ridged_fbm2((float)gx * 0.0020f, (float)gz * 0.0020f, 4, 2.0f, 0.5f, 1.0f, seed + 5003);
    const float dryness = 0.55f * d1 + 0.45f * (1.0f - m1);
    return dryness > 0.52f ? kDesert : kForest;
}
YCGE_HD int choose_surface_block(int biome, int height_y_, int sea, int snow, float slope01)          // Layering.cs:7-28
{
    if (height_y_ >= snow) return kSnow;
    const int d = height_y_ - sea;
    if ((d < 0 ? -d : d) <= kBeachBuffer) return kSand;
    if (slope01 > 0.80f) return kStone;
    switch (biome) {
    case kDesert: return kSand;
    case kAlpine: return slope01 > 0.60f ? kStone : kGrass;
    default: return kGrass;
    }
}
YCGE_HD int choose_subsurface_block(int biome, int gy, int ground_y, int sea)          // Layering.cs:30-45
{
    if (ground_y <= sea + kUnderwaterSandBuffer) return kSand;
    if (biome == kDesert) return kSand;
    const int depth = ground_y - gy;
    if (depth <= kIslandDirtDepth) return kDirt;
    return kStone;
}
// StrataMap.RockMetaAt, :8-19, in its two halves: the noise verdict of the column ...
YCGE_HD int rock_verdict(int gx, int gz, const World &W)
{
    const float n = fbm2((float)gx * 0.004f, (float)gz * 0.004f, 3, 2.0f, 0.5f, 1.0f, W.seed + 4201);
    if (n < 0.33f) return 0;
    if (n < 0.66f) return 1;
    return 2;
}
// ... and the altitude band it falls back to
YCGE_HD int rock_meta(int verdict, int gy)
{
    if (verdict < 2) return verdict;
    const float h_band = (float)(gy % 24) / 24.0f;
    return h_band < 0.33f ? 0 : (h_band < 0.66f ? 1 : 2);
}

// ---------------------------------------------------------------------------------------------------------------- WorldGenerator.cs
// :125-154 for column (lx, lz) of chunk column (cx, cz).  `carved`: the ground after RiverNetwork, index lx * S + lz.
YCGE_HD ColRec column_record(const int *carved, int S, int lx, int lz, int gx, int gz, int river_water, const World &W)
{
    const int x0 = lx - 1 > 0 ? lx - 1 : 0, x1 = lx + 1 < S - 1 ? lx + 1 : S - 1;          // clamped at the chunk's edges, :130-131
    const int z0 = lz - 1 > 0 ? lz - 1 : 0, z1 = lz + 1 < S - 1 ? lz + 1 : S - 1;
    const float dx = (float)(carved[x1 * S + lz] - carved[x0 * S + lz]) * 0.5f;
    const float dz = (float)(carved[lx * S + z1] - carved[lx * S + z0]) * 0.5f;
    const float g = cs_sqrt(dx * dx + dz * dz);
    ColRec R;
    R.slope = clamp01(g / kSlopeNormalize);
    R.ground = carved[lx * S + lz];
    int biome = biome_evaluate(gx, gz, R.ground, W.sea, W);
    const int inland = local_water_y(gx, gz, W, R.ground, R.slope);
    R.water = inland > river_water ? inland : river_water;
    if (R.water > W.sea && R.ground <= R.water) biome = kLakes;
    R.biome_rock = biome | (rock_verdict(gx, gz, W) << 8);
    return R;
}
// :164-195, one cell
YCGE_HD void cell_at(const ColRec &R, int gy, const World &W, int *mat, int *meta)
{
    const int gY = R.ground, wY = R.water, biome = R.biome_rock & 0xff;
    *meta = 0;
    if (gy > gY) *mat = gy <= wY ? kWater : kAir;
    else if (gy == gY) {
        if (wY > W.sea && (wY - gY) <= kBeachBuffer) *mat = kSand;
        else *mat = choose_surface_block(biome, gY, W.sea, W.snow, R.slope);
    }
    else if (gy >= gY - kTerrainDirtDepth) *mat = choose_subsurface_block(biome, gy, gY, W.sea);
    else { *mat = kStone; *meta = rock_meta(R.biome_rock >> 8, gy); }
}

// ---------------------------------------------------------------------------------------------------------------- FloraPlacer.cs
YCGE_HD uint32_t flora_hash(int x, int z, int seed)          // :7-16
{
    uint32_t h = fast_hash(x, 0, z, seed);
    h ^= h << 13; h ^= h >> 17; h ^= h << 5;
    return h;
}
struct Tree {
    int lx, lz;
    int trunk_base, trunk_h, canopy_r, canopy_base;
    int conifer;
};
// :33-69 - does column (lx, lz) of chunk cy carry a tree, and which
YCGE_HD bool tree_at(const ColRec &R, int lx, int lz, int gx, int gz, int base_y, const World &W, Tree *T)
{
    const int S = W.size, b = R.biome_rock & 0xff;
    const int ly_top = R.ground - base_y;
    if (ly_top < 0 || ly_top >= S) return false;
    if (R.ground <= R.water) return false;
    if (R.ground >= W.snow - 2) return false;
    if (R.slope > 0.45f) return false;
    const float density = b == kForest ? 0.03f : 0.0f;
    if (density <= 0.0f) return false;
    const uint32_t h = flora_hash(gx, gz, W.seed + 90001);
    const float r = (float)(h & 0xFFFFu) / 65535.0f;
    if (r > density) return false;
    const bool conifer = b == kTaiga || ((h >> 16) & 3u) == 0u;
    T->lx = lx; T->lz = lz; T->conifer = conifer ? 1 : 0;
    T->trunk_base = ly_top + 1;
    int trunk_h = conifer ? 6 + (int)((h >> 2) & 7u) : 4 + (int)((h >> 3) & 5u);
    T->canopy_r = conifer ? 2 : 2 + (int)((h >> 6) & 1u);
    const int desired_top = T->trunk_base + trunk_h - (conifer ? 2 : 1) + 2;
    if (desired_top > S - 1) {
        const int over = desired_top - (S - 1);
        trunk_h = trunk_h - over > 3 ? trunk_h - over : 3;
    }
    T->trunk_h = trunk_h;
    T->canopy_base = T->trunk_base + trunk_h - (conifer ? 2 : 1);
    return true;
}
YCGE_HD int tree_dy_min(const Tree &T) { return T.conifer ? 0 : -1; }          // :86 (dy runs to 2 for both)
YCGE_HD int tree_radius(const Tree &T, int dy)                                // :90
{
    if (T.conifer) { const int a = T.canopy_r - (dy < 0 ? -dy : dy); return a > 1 ? a : 1; }
    return T.canopy_r - (dy == 2 ? 1 : 0);
}
YCGE_HD bool tree_may_replace(int mat) { return mat == kAir || mat == kTallGrass; }          // :76, :101

}  // namespace wg
}  // namespace ycge
