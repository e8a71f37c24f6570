// ycge_worldgen.h - WorldGenerator.GenerateChunkCells and WorldManager.GenerateAndSaveWorld restated for host and gfx950
// (Scenes/WorldGeneration/*.cs of the reference).
//
// One chunk of the voxel world is a pure function of (cx, cy, cz, WorldConfig): integer hashing and fp32 + - * / sqrt floor round, plus
// one MathF.Pow.  Everything here obeys ycge_math.h's contract (no contraction, correctly rounded divide and sqrt, m_pow for the power), so
// the host generator (ycge_worldgen.cpp) and the kernels (ycge_worldgen.hip) give the same cells, bit for bit.
//
// IslandSettings (IslandSettings.cs:5-54) and the WorldGenSettings fields the generator reads (WorldGenSettings.cs) are compile-time
// constants at the reference's values.  Not restated: the dead FBM3D / GradientNoise3D / GetBlockAt, SimpleEntityPlacer.
//
// The work is cut where the data flow cuts it:
//   height_y            TerrainNoise.HeightY: once per cell of the (S + 2)^2 tile around a chunk column (cx, cz)
//   d8_direction        RiverNetwork.cs:31-56, from the tile
//   river_accum         RiverNetwork.cs:58-78 (see there: an in-degree count)
//   river_carve         RiverNetwork.cs:80-113
//   column_record       WorldGenerator.cs:125-154 + StrataMap's noise verdict: what every cy of the column shares
//   cell_at             WorldGenerator.cs:156-199, one cell from its column's record
//   tree_at + the tree_* helpers   FloraPlacer.cs:27-69; the placement loops (:71-131) are the callers'
// and, for the whole-world pregen (WorldManager.cs:510-631; the second half of this file):
//   d8_global, river_accum_global   RiverNetworkGlobal.cs:17-63 over the window
//   column_record_global            WorldManager.cs:543-559
//   cell_at_global                  WorldManager.cs:569-598
//   feature_at, feature_write       FloraPlacer.PlaceTreesGlobal (:137-254) as one descriptor per column and its write set
//   world_cell_before, world_cell, tree_any_leaves   the serial placement as a gather
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

// ================================================================================================================ the whole-world pregen
// WorldManager.GenerateAndSaveWorld over a window of nx x nz columns whose column (x, z) is block (ox + x, oz + z) of the world in every
// noise, hash and strata call; every clamp and bound is the window's.  ox = oz = 0 is the reference.  Fields are indexed x * nz + z.
struct Window {
    int nx, nz;          // ChunksX * ChunkSize, ChunksZ * ChunkSize
    int ox, oz;
};
constexpr float kRiverBankSand = 1.5f;          // IslandSettings.cs:54
constexpr int kFeatReach = 3;                   // a feature writes at most 3 columns from its root (a broadleaf canopy of radius 3)

// RiverNetworkGlobal.cs:17-40 - as d8_direction, but a neighbour outside the window is skipped (:29)
YCGE_HD int d8_global(const int *ground, int nx, int nz, int x, int z)
{
    const int h0 = ground[x * nz + z];
    int best_dx = 0, best_dz = 0, best_drop = 0;
    for (int oz = -1; oz <= 1; oz++)
        for (int ox = -1; ox <= 1; ox++) {
            if (ox == 0 && oz == 0) continue;
            const int x2 = x + ox, z2 = z + oz;
            if (x2 < 0 || x2 >= nx || z2 < 0 || z2 >= nz) continue;
            const int drop = h0 - ground[x2 * nz + z2];
            if (drop > best_drop) { best_drop = drop; best_dx = ox; best_dz = oz; }
        }
    return (best_dx + 1) * 3 + (best_dz + 1);
}
// RiverNetworkGlobal.cs:42-63.  The argument of river_accum carries over: cells are visited by height ASCENDING, a cell drains into a
// STRICTLY lower cell (bestDrop > 0), which the order has already passed, so when a cell is visited nothing has reached it yet: a is 0,
// is raised to 1 (:55), and every draining cell adds exactly 1 to its target.  Array.Sort's order among equal heights cannot matter (equal
// cells never drain into each other).  Unlike the per-chunk pass, a cell with no lower neighbour adds nothing (:58), and a D8 target is in
// the window by construction.  accum is therefore the number of neighbours whose D8 points at the cell: at most 8, far from the
// threshold of 50 - nothing is ever carved, and the river surface is the sea everywhere.
YCGE_HD float river_accum_global(const uint8_t *dir, int nx, int nz, int x, int z)
{
    int n = 0;
    for (int ox = -1; ox <= 1; ox++)
        for (int oz = -1; oz <= 1; oz++) {
            if (ox == 0 && oz == 0) continue;
            const int x2 = x + ox, z2 = z + oz;
            if (x2 < 0 || x2 >= nx || z2 < 0 || z2 >= nz) continue;
            if (dir[x2 * nz + z2] == (1 - ox) * 3 + (1 - oz)) n++;
        }
    return (float)n;
}
// RiverNetworkGlobal.cs:65-83 with WorldManager.cs:536 is river_carve: Math.Max(0, ground - floor(carve)) is ground where floor(carve) is 0.

// WorldManager.cs:543-559 for column (x, z).  `carved`: the ground after the river pass.
YCGE_HD ColRec column_record_global(const int *carved, const Window &N, int x, int z, int river_water, const World &W)
{
    const int nx = N.nx, nz = N.nz;
    const int x0 = x - 1 > 0 ? x - 1 : 0, x1 = x + 1 < nx - 1 ? x + 1 : nx - 1;          // clamped at the window's edges, :547-548
    const int z0 = z - 1 > 0 ? z - 1 : 0, z1 = z + 1 < nz - 1 ? z + 1 : nz - 1;
    const float dx = (float)(carved[x1 * nz + z] - carved[x0 * nz + z]) * 0.5f;
    const float dz = (float)(carved[x * nz + z1] - carved[x * nz + z0]) * 0.5f;
    const float g = cs_sqrt(dx * dx + dz * dz);
    const int gx = N.ox + x, gz = N.oz + z;
    ColRec R;
    R.slope = clamp01(g / kSlopeNormalize);
    R.ground = carved[x * nz + z];
    int biome = biome_evaluate(gx, gz, R.ground, W.sea, W);
    const int inland = local_water_y(gx, gz, W, R.ground, R.slope);
    R.water = inland > river_water ? inland : river_water;
    if (R.water > W.sea && R.ground <= R.water) biome = kLakes;
    R.biome_rock = biome | (rock_verdict(gx, gz, W) << 8);
    return R;
}
// WorldManager.cs:569-598, one cell: cell_at with the bank rule of :580, an int compared with 3.5f
YCGE_HD void cell_at_global(const ColRec &R, int gy, const World &W, int *mat, int *meta)
{
    const int gY = R.ground, wY = R.water, biome = R.biome_rock & 0xff;
    *meta = 0;
    if (gy > gY) *mat = gy <= wY ? kWater : kAir;
    else if (gy == gY) {
        if (wY > W.sea && (float)(wY - gY) <= (float)kBeachBuffer + kRiverBankSand) *mat = kSand;
        else *mat = choose_surface_block(biome, gY, W.sea, W.snow, R.slope);
    }
    else if (gy >= gY - kTerrainDirtDepth) *mat = choose_subsurface_block(biome, gy, gY, W.sea);
    else { *mat = kStone; *meta = rock_meta(R.biome_rock >> 8, gy); }
}

// ---- FloraPlacer.PlaceTreesGlobal as data.  Forest and Desert exclude each other, so a column roots at most one feature:
//   bits 0-1   kind: 0 none, 1 tree, 2 cactus, 3 rock pile
//   tree:      bit 2 conifer, bits 3-7 trunkH after the clip at the world's top (:168-169; <= 13), bits 8-9 canopyR
//   cactus:    bits 3-5 height (2..5)
// A feature stands on its column's ground (trunkBase = gY + 1), which the column's record holds.
enum : uint32_t { kFeatNone = 0, kFeatTree = 1, kFeatCactus = 2, kFeatRock = 3 };
YCGE_HD uint32_t feature_at(const ColRec &R, int gx, int gz, const World &W)
{
    const int gY = R.ground, wY = R.water, b = R.biome_rock & 0xff, ny = W.height;
    if (b == kForest) {          // :150-169 (density is 0 for every other biome; no slope test here)
        if (gY <= wY || gY >= W.snow - 2) return kFeatNone;
        const uint32_t h = flora_hash(gx, gz, W.seed + 90001);
        const float r = (float)(h & 0xFFFFu) / 65535.0f;
        if (r > 0.03f) return kFeatNone;
        const bool conifer = ((h >> 16) & 3u) == 0u;
        const int trunk_base = gY + 1;
        int trunk_h = conifer ? 6 + (int)((h >> 2) & 7u) : 4 + (int)((h >> 3) & 5u);
        const int canopy_r = conifer ? 2 : 2 + (int)((h >> 6) & 1u);
        if (trunk_base + trunk_h + 2 >= ny) trunk_h = ny - trunk_base - 2 > 3 ? ny - trunk_base - 2 : 3;
        return kFeatTree | (conifer ? 4u : 0u) | ((uint32_t)trunk_h << 3) | ((uint32_t)canopy_r << 8);
    }
    if (b == kDesert) {          // :216-225
        if (gY <= wY) return kFeatNone;
        if (R.slope > 0.25f) return kFeatNone;
        const uint32_t ux = (uint32_t)gx, uz = (uint32_t)gz;          // (C# int products wrap; so do these)
        const uint32_t h = flora_hash((int)((ux * 73856093u) ^ (uz * 19349663u)), (int)((uz * 83492791u) ^ (ux * 297121507u)), W.seed + 1234567);
        const float r = (float)(h & 0xFFFFu) / 65535.0f;
        if (r < 0.70f) return kFeatNone;
        if (r < 0.85f) return kFeatCactus | ((2u + ((h >> 16) & 3u)) << 3);
        return kFeatRock;
    }
    return kFeatNone;
}
YCGE_HD int feat_kind(uint32_t d) { return (int)(d & 3u); }
YCGE_HD int feat_trunk_h(uint32_t d) { return (int)((d >> 3) & 31u); }
YCGE_HD int feat_cactus_h(uint32_t d) { return (int)((d >> 3) & 7u); }
YCGE_HD Tree feat_tree(uint32_t d, int gY)          // (lx, lz unused; canopy_base as :178)
{
    Tree T;
    T.lx = T.lz = 0;
    T.conifer = (d >> 2) & 1u; T.trunk_h = feat_trunk_h(d); T.canopy_r = (int)((d >> 8) & 3u);
    T.trunk_base = gY + 1;
    T.canopy_base = T.trunk_base + T.trunk_h - (T.conifer ? 2 : 1);
    return T;
}
// the highest y a feature may write (trunk top and canopy top; a crown lies at the trunk top), for the fill's early out
YCGE_HD int feat_top(uint32_t d, int gY)
{
    switch (feat_kind(d)) {
    case kFeatTree: return feat_tree(d, gY).canopy_base + 2;
    case kFeatCactus: return gY + feat_cactus_h(d);
    case kFeatRock: return gY + 1;
    default: return gY;
    }
}
// One feature's turn at the cell (dx, y, dz) from its root, whose material so far is *mat: trunk, then canopy, then the fallback crown
// (:171-211), or the cactus (:229-234), or the rock pile (:239-250), each with its own rule for what it may replace.  The cell lies in
// the window and below the world's top, so the x2 / z2 / y bounds of the C# hold (trunkBase >= 1: y < 0 never happens; the trunk's and
// the cactus' `break` at the top ends a loop whose later y are higher still).
YCGE_HD void feature_write(uint32_t d, int gY, bool fallback, int dx, int y, int dz, int *mat, int *meta)
{
    const int adx = dx < 0 ? -dx : dx, adz = dz < 0 ? -dz : dz;
    switch (feat_kind(d)) {
    case kFeatTree: {
        const Tree T = feat_tree(d, gY);
        if (adx == 0 && adz == 0 && y >= T.trunk_base && y < T.trunk_base + T.trunk_h && tree_may_replace(*mat)) { *mat = kWood; *meta = 0; }
        const int dy = y - T.canopy_base;
        if (dy >= tree_dy_min(T) && dy <= 2) {
            const int radius = tree_radius(T, dy);
            if (adx <= radius && adz <= radius && tree_may_replace(*mat)) { *mat = kLeaves; *meta = 0; }
        }
        if (fallback && y == T.trunk_base + T.trunk_h - 1 && adx <= 1 && adz <= 1 && *mat == kAir) { *mat = kLeaves; *meta = 0; }
        break;
    }
    case kFeatCactus:
        if (adx == 0 && adz == 0 && y > gY && y <= gY + feat_cactus_h(d) && *mat == kAir) { *mat = kWood; *meta = 0; }
        break;
    case kFeatRock:
        if (y == gY + 1 && adx + adz <= 1 && *mat == kAir) { *mat = kStone; *meta = 1; }
        break;
    default: break;
    }
}
// The cell (x, y, z) as PlaceTreesGlobal has left it just BEFORE the canopy of the tree rooted at (lim_x, lim_z): the base cell, then the
// features rooted within kFeatReach columns in the serial order - x-row by x-row, a row's trees in z order, then that row's desert
// features in z order - up to and excluding that tree (its own row's desert pass comes after it).  Every write leaves the cell neither Air
// nor TallGrass, which no feature replaces, so the scan ends at the first one.  `fallback`: one flag per column, read for trees only.
YCGE_HD void world_cell_before(const ColRec *rec, const uint32_t *feat, const uint8_t *fallback, const Window &N, const World &W, int x, int y, int z,
                               int lim_x, int lim_z, int *mat, int *meta)
{
    cell_at_global(rec[x * N.nz + z], y, W, mat, meta);
    if (!tree_may_replace(*mat)) return;
    const int fx0 = x - kFeatReach > 0 ? x - kFeatReach : 0, fx_hi = x + kFeatReach < N.nx - 1 ? x + kFeatReach : N.nx - 1, fx1 = fx_hi < lim_x ? fx_hi : lim_x;
    const int fz0 = z - kFeatReach > 0 ? z - kFeatReach : 0, fz1 = z + kFeatReach < N.nz - 1 ? z + kFeatReach : N.nz - 1;
    for (int fx = fx0; fx <= fx1; fx++) {
        for (int pass = 0; pass < 2; pass++) {          // 0: the row's trees, 1: its desert features
            if (pass == 1 && fx == lim_x) break;
            for (int fz = fz0; fz <= fz1; fz++) {
                if (pass == 0 && fx == lim_x && fz >= lim_z) break;
                const uint32_t d = feat[fx * N.nz + fz];
                if (d == kFeatNone || (feat_kind(d) == kFeatTree) != (pass == 0)) continue;
                feature_write(d, rec[fx * N.nz + fz].ground, fallback[fx * N.nz + fz] != 0, x - fx, y, z - fz, mat, meta);
                if (!tree_may_replace(*mat)) return;
            }
        }
    }
}
// the finished cell: no limit
YCGE_HD void world_cell(const ColRec *rec, const uint32_t *feat, const uint8_t *fallback, const Window &N, const World &W, int x, int y, int z, int *mat, int *meta)
{
    world_cell_before(rec, feat, fallback, N, W, x, y, z, 0x7fffffff, 0, mat, meta);
}
// anyLeaves of the tree rooted at (x, z) (:179-195): did its canopy loop find a cell it could take?  The cell as the earlier features and
// the tree's own trunk left it.  Depends on the fallback flags of EARLIER trees only.
YCGE_HD bool tree_any_leaves(const ColRec *rec, const uint32_t *feat, const uint8_t *fallback, const Window &N, const World &W, int x, int z)
{
    const uint32_t d = feat[x * N.nz + z];
    const Tree T = feat_tree(d, rec[x * N.nz + z].ground);
    for (int dy = tree_dy_min(T); dy <= 2; dy++) {
        const int y = T.canopy_base + dy;
        if (y < 0 || y >= W.height) continue;
        const int radius = tree_radius(T, dy);
        for (int rx = -radius; rx <= radius; rx++) {
            const int x2 = x + rx;
            if (x2 < 0 || x2 >= N.nx) continue;
            for (int rz = -radius; rz <= radius; rz++) {
                const int z2 = z + rz;
                if (z2 < 0 || z2 >= N.nz) continue;
                int mat, meta;
                world_cell_before(rec, feat, fallback, N, W, x2, y, z2, x, z, &mat, &meta);
                if (rx == 0 && rz == 0 && y >= T.trunk_base && y < T.trunk_base + T.trunk_h && tree_may_replace(mat)) mat = kWood;
                if (tree_may_replace(mat)) return true;
            }
        }
    }
    return false;
}

}  // namespace wg
}  // namespace ycge
