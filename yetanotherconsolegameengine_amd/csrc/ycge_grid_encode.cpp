// ycge_grid_encode.cpp - chunk streaming: ycge_scene_attach_grids / ycge_scene_detach_grids and the pool of resident voxel grids.
//
// The reference's voxel world attaches and removes VolumeGrids every frame (VolumeScene.Update -> WorldManager.LoadChunksAround,
// Scenes/VolumeScenes.cs:63-64, WorldManager.cs:289-370).  An attach brings the raw cells of its grids up once through page-locked
// staging; k_grid_encode (ycge_grid_encode.hip) writes the bricked bytes, the solid box, the brick mask and the "no material" verdict of
// the whole batch in one launch, and one small read-back tells the host what flatten_objects needs.  Grids whose lookup table exceeds
// YCGE_ENC_MAX_LOOKUP entries take the host encoder of ycge_scene_upload.
//
// ALL OR NOTHING: every step works on a copy of the pool (GridPool) and writes only slots, arena blocks and LUT regions no resident grid
// owns; the copy replaces the pool in a last step that cannot fail.  The arena grows only after every verdict is in, so a refused attach
// leaves the arena's capacity and the pool's counters as they were.  (The LUT and the grid table may have grown, contents kept, and the
// staging and scratch buffers stay: none of it is observable, nothing refers to the new room.)
//
// VERDICTS: a grid that is wrong in two ways - a pair with no material AND more than 255 distinct pairs - is refused as "no material"
// (YCGE_ERR_INVALID_ARG) here, where ycge_scene_upload reports whichever its z-outer walk meets first.
//
// SEVERAL DEVICES: every device of a multi-device context gets the batch by a copy, a launch and a read-back of its own, one device
// after the other - an attach is serial in the number of devices; last_attach_us times the root's share.
//
// FRAMES IN FLIGHT: an attach joins them (quiesce), as every other scene change does - it may move the arena, the LUT and the grid table,
// which the frames read.  A detach changes host state only and joins nothing.
#include <algorithm>
#include <climits>
#include <map>
#include <unordered_set>

#include "ycge_ctx.h"
#include "ycge_grid_encode.h"
#include "ycge_worldgen_host.h"

namespace ycge_host {

void grid_pool_reset(ycge_ctx *c, const std::vector<GGrid> &recs, size_t arena_bytes, size_t lut_entries)
{
    GridPool P;
    const size_t n = recs.size();
    P.recs = recs;
    P.resident.assign(n, 1);
    P.block_bytes.assign(n, 0);
    P.lut_region.assign(n, -1);
    P.owner.assign(n, -1);
    for (size_t i = 0; i < n; i++) {
        P.block_bytes[i] = (uint32_t)((size_t)recs[i].nbx * recs[i].nby * recs[i].nbz * 512);
        P.arena_in_use += P.block_bytes[i];
    }
    P.arena_end = arena_bytes; P.lut_end = lut_entries; P.n_resident = (int64_t)n;
    c->grid_pool = std::move(P);
}

namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

int morton3_host(int x, int y, int z)
{
    return ((x & 1) << 0) | ((y & 1) << 1) | ((z & 1) << 2) | ((x & 2) << 2) | ((y & 2) << 3) | ((z & 2) << 4) | ((x & 4) << 4) | ((y & 4) << 5) | ((z & 4) << 6);
}

// room for `need` elements with the first `keep` preserved (device to device): the one place that copies resident bytes
template <class T> hipError_t grow_preserve(DevBuf<T> &b, size_t need, size_t keep)
{
    if (need <= b.cap) { if (b.n < need) b.n = need; return hipSuccess; }
    DevBuf<T> nb;
    hipError_t e = nb.alloc(need);
    if (e != hipSuccess) return e;
    if (keep && b.p) {
        e = hipMemcpy(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return e;
    }
    b = std::move(nb);
    return hipSuccess;
}

// the calling thread's current device goes back to the root's on every way out (a failed step on a peer's device included)
struct DeviceGuard {
    int device;
    explicit DeviceGuard(int d) : device(d) {}
    ~DeviceGuard() { (void)hipSetDevice(device); }
};

struct Planned {
    int32_t index = -1;
    uint32_t off = 0, cap = 0;          // block of the cell arena
    uint32_t lut = 0;                   // first entry of the LUT region
    bool device = true;                 // k_grid_encode (else the host encoder)
    bool direct = true;                 // the block lies inside the arena as it is: the kernel writes it in place
    size_t scratch_off = 0;             // ... else into d_enc_out here, copied once the arena has grown
    size_t cells_off = 0, lookup_off = 0;   // in the staged batch
    GGrid rec;
    std::vector<uint8_t> host_bytes;    // host encoder: the bricked bytes and the table
    std::vector<int32_t> host_lut;
};

double us_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }

// ycge_scene_generate_grids: where the cells of grid k come from when no caller brought them
struct GenSource {
    wg::World W;
    bool host = false;                               // YCGE_WORLDGEN_HOST: ycge_worldgen.cpp fills the staging, the rest is an attach
    std::vector<std::array<int32_t, 3>> keys;        // per grid
    std::vector<int32_t> col;                        // per grid: its chunk column among the column records
    std::vector<wg::ColRec> host_cols;               // host: n_cols x S * S (device: every context's d_wg_cols)
    std::vector<int32_t *> cells_out;                // per grid, or empty
    // ycge_scene_generate_world: keys are chunk coordinates in the window; the cells come from the window's fields on every device
    // (k_wp_fill), or are slices of host_world
    bool world = false;
    wg::Window N{};
    const int32_t *host_world = nullptr;             // host: the whole world's cells, VG01 order
    int32_t *world_out = nullptr;                    // device: the caller's cells_out (whole world), or NULL
    size_t chunk_bytes() const { return (size_t)W.size * W.size * W.size * 8; }
};
// chunk `key` of a world in VG01 order <-> its S^3 cells in ycge_grid.cells order (rows of S cells along z)
void world_slice(const GenSource &g, const std::array<int32_t, 3> &key, const int32_t *world, int32_t *chunk)
{
    const size_t S = (size_t)g.W.size, ny = (size_t)g.W.height, nz = (size_t)g.N.nz;
    for (size_t lx = 0; lx < S; lx++)
        for (size_t ly = 0; ly < S; ly++)
            std::memcpy(chunk + 2 * (lx * S + ly) * S, world + 2 * (((key[0] * S + lx) * ny + key[1] * S + ly) * nz + key[2] * S), S * 8);
}
void world_scatter(const GenSource &g, const std::array<int32_t, 3> &key, const int32_t *chunk, int32_t *world)
{
    const size_t S = (size_t)g.W.size, ny = (size_t)g.W.height, nz = (size_t)g.N.nz;
    for (size_t lx = 0; lx < S; lx++)
        for (size_t ly = 0; ly < S; ly++)
            std::memcpy(world + 2 * (((key[0] * S + lx) * ny + key[1] * S + ly) * nz + key[2] * S), chunk + 2 * (lx * S + ly) * S, S * 8);
}
// where the fields of a window of n columns (and the occupancy words of its n_chunks chunks, last: nothing else moves with their number)
// lie in a context's d_wg_cols
size_t wp_layout(uint8_t *base, size_t n, size_t n_chunks, WpFields *F)
{
    size_t at = 0;
    auto take = [&](size_t bytes) { uint8_t *p = base ? base + at : nullptr; at = align_up(at + bytes, 256); return p; };
    WpFields f;
    f.rec = (wg::ColRec *)take(n * sizeof(wg::ColRec));
    f.ground0 = (int32_t *)take(n * 4); f.ground = (int32_t *)take(n * 4); f.river_water = (int32_t *)take(n * 4);
    f.feat = (uint32_t *)take(n * 4); f.reach = (int32_t *)take(n * 4);
    f.dir = take(n); f.fallback = take(n);
    (void)take(n);          // the other flag buffer of the anyLeaves passes (wp_next_flags)
    f.changed = (uint32_t *)take(256);
    f.occupied = (uint32_t *)take(n_chunks * 4);
    if (F) *F = f;
    return at;
}
uint8_t *wp_next_flags(const WpFields &F, size_t n) { return F.fallback + align_up(n, 256); }
constexpr size_t kGenGroupMax = 32768;               // chunks in one fill launch (gridDim.y)

// one group of device-encoded grids: stage, copy, launch, read back (every device of the context; the root's results are returned).
// With a device GenSource nothing but descriptors and lookup tables is staged: k_wg_fill / k_wg_trees write the cells where k_grid_encode reads them.
int encode_group(ycge_ctx *root, const ycge_grid *grids, std::vector<Planned> &plan, const std::vector<int> &group, std::vector<GridEncResult> &res, double us[4],
                 const GenSource *gen)
{
    const DeviceGuard guard(root->device);
    const size_t m = group.size();
    const bool gen_dev = gen && !gen->host;
    size_t at = align_up(m * sizeof(GridEncDesc), 256);
    const size_t off_res = at;
    at = align_up(at + m * sizeof(GridEncResult), 256);
    const size_t off_chunks = at;
    if (gen_dev) at = align_up(at + m * sizeof(WgChunk), 256);
    const size_t off_any = at;
    if (gen_dev) at = align_up(at + m * sizeof(uint32_t), 256);
    for (int k : group) { plan[k].lookup_off = at; at = align_up(at + (size_t)grids[k].n_lookup * sizeof(ycge_voxel_lookup), 16); }
    at = align_up(at, 256);
    const size_t off_cells = at;
    for (int k : group) { plan[k].cells_off = at; at = align_up(at + (size_t)grids[k].nx * grids[k].ny * grids[k].nz * 8, 256); }
    const size_t dev_total = at;                                                    // what the device holds
    const size_t up_bytes = gen_dev ? off_cells : at;                               // what goes up
    const size_t off_back = up_bytes, back_bytes = m * sizeof(GridEncResult) + (gen_dev ? m * sizeof(uint32_t) : 0);   // (staging only)
    HIP_TRY(root, root->enc_stage.reserve(off_back + back_bytes, hipHostMallocPortable));      // (every device of the context copies from it)
    uint8_t *st = root->enc_stage.data();
    auto t0 = std::chrono::steady_clock::now();
    GridEncResult *init = (GridEncResult *)(st + off_res);
    uint32_t n_wg = 0;
    std::vector<uint32_t> first_wg(m);
    for (size_t j = 0; j < m; j++) {
        const ycge_grid &g = grids[group[j]];
        const Planned &pl = plan[group[j]];
        GridEncResult r;
        std::memset(&r, 0, sizeof r);
        r.lo[0] = g.nx; r.lo[1] = g.ny; r.lo[2] = g.nz; r.hi[0] = r.hi[1] = r.hi[2] = -1; r.bad_cell = 0xffffffffu;
        init[j] = r;
        if (g.n_lookup > 0) std::memcpy(st + pl.lookup_off, g.lookup, (size_t)g.n_lookup * sizeof(ycge_voxel_lookup));
        if (!gen) std::memcpy(st + pl.cells_off, g.cells, (size_t)g.nx * g.ny * g.nz * 8);
        else if (gen->world && gen->host) {
            const size_t k = (size_t)group[j];
            world_slice(*gen, gen->keys[k], gen->host_world, (int32_t *)(st + pl.cells_off));
        } else if (gen->host) {
            const size_t k = (size_t)group[j];
            int32_t any = 0;
            worldgen_fill_host(gen->W, gen->host_cols.data() + (size_t)gen->col[k] * gen->W.size * gen->W.size, gen->keys[k][0], gen->keys[k][1], gen->keys[k][2],
                               (int32_t *)(st + pl.cells_off), &any);
            if (!any) return root->fail(YCGE_ERR_INTERNAL, "ycge_scene_generate_grids: chunk (%d, %d, %d) came out empty", gen->keys[k][0], gen->keys[k][1], gen->keys[k][2]);
            if (!gen->cells_out.empty()) std::memcpy(gen->cells_out[k], st + pl.cells_off, gen->chunk_bytes());
        } else ((uint32_t *)(st + off_any))[j] = 0u;
        first_wg[j] = n_wg;
        const uint64_t wgs = (uint64_t)pl.rec.nbx * pl.rec.nby * (((uint64_t)pl.rec.nbz + YCGE_ENC_RUN - 1) / YCGE_ENC_RUN);
        if (n_wg + wgs >= 0x7fffffffull) return root->fail(YCGE_ERR_UNSUPPORTED, "ycge_scene_attach_grids: more bricks in one batch than one launch takes");
        n_wg += (uint32_t)wgs;
    }
    us[0] += us_since(t0);
    std::vector<ycge_ctx *> ctxs{root};
    ctxs.insert(ctxs.end(), root->peers.begin(), root->peers.end());
    for (ycge_ctx *c : ctxs) {
        HIP_TRY(root, hipSetDevice(c->device));
        if (c->d_enc_in.cap < dev_total) HIP_TRY(root, c->d_enc_in.alloc(dev_total));
        GridEncDesc *descs = (GridEncDesc *)st;
        for (size_t j = 0; j < m; j++) {
            const ycge_grid &g = grids[group[j]];
            const Planned &pl = plan[group[j]];
            GridEncDesc d;
            std::memset(&d, 0, sizeof d);
            d.cells = (const int32_t *)(c->d_enc_in.p + pl.cells_off);
            d.out = pl.direct ? c->d_cells.p + pl.off : c->d_enc_out.p + pl.scratch_off;
            d.lut = c->d_lut.p + pl.lut;
            d.lookup = (const int32_t *)(c->d_enc_in.p + pl.lookup_off);
            d.nx = g.nx; d.ny = g.ny; d.nz = g.nz; d.nbx = pl.rec.nbx; d.nby = pl.rec.nby; d.nbz = pl.rec.nbz;
            d.n_lookup = g.n_lookup;
            d.default_material = (g.default_material >= 0 && g.default_material < root->n_materials) ? g.default_material : -1;
            d.first_wg = first_wg[j];
            d.maskable = pl.rec.has_brick_mask ? 1u : 0u;
            descs[j] = d;
            if (gen_dev) {
                const size_t k = (size_t)group[j];
                WgChunk w;
                w.cx = gen->keys[k][0]; w.cy = gen->keys[k][1]; w.cz = gen->keys[k][2]; w.col = gen->col[k];
                w.cells = (int32_t *)(c->d_enc_in.p + pl.cells_off);
                ((WgChunk *)(st + off_chunks))[j] = w;
            }
        }
        t0 = std::chrono::steady_clock::now();
        HIP_TRY(root, hipMemcpyAsync(c->d_enc_in.p, st, up_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(root, hipStreamSynchronize(c->stream));
        if (c == root) us[1] += us_since(t0);
        t0 = std::chrono::steady_clock::now();
        if (gen_dev) {
            int ge;
            if (gen->world) {
                WpFields F;
                wp_layout(c->d_wg_cols.p, (size_t)gen->N.nx * gen->N.nz, 0, &F);
                ge = ycge_launch_worldpregen_fill((const WgChunk *)(c->d_enc_in.p + off_chunks), (int)m, &gen->W, &gen->N, &F, (uint32_t *)(c->d_enc_in.p + off_any), c->stream);
            } else
                ge = ycge_launch_worldgen_fill((const WgChunk *)(c->d_enc_in.p + off_chunks), (int)m, &gen->W, (const wg::ColRec *)c->d_wg_cols.p,
                                               (uint32_t *)(c->d_enc_in.p + off_any), c->stream);
            if (ge != 0) return root->fail(YCGE_ERR_DEVICE, "%s launch failed: %s", gen->world ? "k_wp_fill" : "k_wg_fill", hipGetErrorString((hipError_t)ge));
            if (c == root) { HIP_TRY(root, hipStreamSynchronize(c->stream)); root->worldgen_last_us[1] += us_since(t0); t0 = std::chrono::steady_clock::now(); }
        }
        const int e = ycge_launch_grid_encode(c->d_enc_in.p, (int)m, c->d_enc_in.p + off_res, n_wg, c->stream);
        if (e != 0) return root->fail(YCGE_ERR_DEVICE, "k_grid_encode launch failed: %s", hipGetErrorString((hipError_t)e));
        HIP_TRY(root, hipStreamSynchronize(c->stream));
        if (c == root) us[2] += us_since(t0);
        t0 = std::chrono::steady_clock::now();
        HIP_TRY(root, hipMemcpyAsync(st + off_back, c->d_enc_in.p + off_res, m * sizeof(GridEncResult), hipMemcpyDeviceToHost, c->stream));
        if (gen_dev) HIP_TRY(root, hipMemcpyAsync(st + off_back + m * sizeof(GridEncResult), c->d_enc_in.p + off_any, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(root, hipStreamSynchronize(c->stream));
        if (c == root) {
            us[3] += us_since(t0);
            for (size_t j = 0; j < m; j++) std::memcpy(&res[(size_t)group[j]], st + off_back + j * sizeof(GridEncResult), sizeof(GridEncResult));
        }
        if (gen_dev && c == root) {
            const uint32_t *any = (const uint32_t *)(st + off_back + m * sizeof(GridEncResult));
            std::vector<uint8_t> made;          // ycge_scene_generate_world with cells_out: the group's cell area in ONE copy, scattered below
            if (gen->world && gen->world_out) {
                made.resize(dev_total - off_cells);
                const int rc = copy_out(root, made.data(), c->d_enc_in.p + off_cells, made.size());
                if (rc != YCGE_OK) return rc;
            }
            for (size_t j = 0; j < m; j++) {
                const size_t k = (size_t)group[j];
                if (!any[j]) return root->fail(YCGE_ERR_INTERNAL, "%s: chunk (%d, %d, %d) came out empty", gen->world ? "ycge_scene_generate_world" : "ycge_scene_generate_grids",
                                               gen->keys[k][0], gen->keys[k][1], gen->keys[k][2]);
                if (!made.empty()) world_scatter(*gen, gen->keys[k], (const int32_t *)(made.data() + (plan[k].cells_off - off_cells)), gen->world_out);
                if (!gen->cells_out.empty()) {
                    const int rc = copy_out(root, gen->cells_out[k], c->d_enc_in.p + plan[k].cells_off, gen->chunk_bytes());
                    if (rc != YCGE_OK) return rc;
                }
            }
        }
    }
    if (gen) {          // a pair with no material: named here, while the group's cells are still where they were made
        for (size_t j = 0; j < m; j++) {
            const size_t k = (size_t)group[j];
            const GridEncResult &r = res[k];
            if (r.bad_cell == 0xffffffffu) continue;
            int32_t pair[2] = {0, 0};
            if (gen->host) std::memcpy(pair, st + plan[k].cells_off + (size_t)r.bad_cell * 8, 8);
            else {
                HIP_TRY(root, hipSetDevice(root->device));
                const int rc = copy_out(root, pair, root->d_enc_in.p + plan[k].cells_off + (size_t)r.bad_cell * 8, 8);
                if (rc != YCGE_OK) return rc;
            }
            return root->fail(YCGE_ERR_INVALID_ARG, "grid %d: no material for (matId %d, metaId %d)", (int)k, pair[0], pair[1]);
        }
    }
    (void)hipSetDevice(root->device);
    return YCGE_OK;
}

// more than 255 distinct (matId, metaId) pairs among the solid cells? (only asked for grids whose cells missed the lookup table)
bool too_many_pairs(const ycge_grid &g)
{
    std::unordered_set<uint64_t> seen;
    const size_t n = (size_t)g.nx * g.ny * g.nz;
    for (size_t i = 0; i < n; i++) {
        if (g.cells[2 * i] <= 0) continue;
        seen.insert(((uint64_t)(uint32_t)g.cells[2 * i] << 32) | (uint32_t)g.cells[2 * i + 1]);
        if (seen.size() > 255) return true;
    }
    return false;
}

}  // namespace
}  // namespace ycge_host

extern "C" {

// the body of ycge_scene_attach_grids (gen == NULL: the caller's cells) and of ycge_scene_generate_grids (the cells of grids[k] are made
// from gen->keys[k]; grids[k].cells is not read).  Arguments are checked by the callers; n >= 1.
static int attach_common(ycge_ctx *c, const ycge_grid *grids, int32_t n, int32_t *out_grid_index, const GenSource *gen)
{
    int rc = quiesce(c);
    for (ycge_ctx *p : c->peers) if (rc == YCGE_OK) rc = quiesce(p);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const DeviceGuard guard(c->device);

    // ---- the plan, on copies: indices (lowest free first), arena blocks (a free block of that size, else the end), LUT regions
    GridPool P = c->grid_pool;
    std::vector<std::array<float, 6>> bounds = c->grid_bounds;
    std::vector<std::array<float, 7>> solid = c->grid_solid;
    std::vector<Planned> plan((size_t)n);
    const size_t arena_cap = c->d_cells.p ? c->d_cells.cap : 0;
    size_t scratch = 0;
    for (int k = 0; k < n; k++) {
        Planned &pl = plan[(size_t)k];
        grid_record_init(grids[k], pl.rec);
        pl.device = grids[k].n_lookup <= YCGE_ENC_MAX_LOOKUP;
        if (!P.free_index.empty()) { pl.index = *P.free_index.begin(); P.free_index.erase(P.free_index.begin()); P.slots_reused++; }
        else {
            pl.index = (int32_t)P.recs.size();
            P.recs.push_back(GGrid{}); P.resident.push_back(0); P.block_bytes.push_back(0); P.lut_region.push_back(-1);
            bounds.push_back(std::array<float, 6>{{0, 0, 0, -1, -1, -1}}); solid.push_back(std::array<float, 7>{});
        }
        pl.cap = (uint32_t)((size_t)pl.rec.nbx * pl.rec.nby * pl.rec.nbz * 512);
        auto fb = P.free_blocks.find(pl.cap);
        if (fb != P.free_blocks.end()) { pl.off = fb->second; P.free_blocks.erase(fb); }
        else {
            const uint64_t off = (P.arena_end + 255) & ~(uint64_t)255;
            if (off + pl.cap >= ((uint64_t)1 << 32)) return c->fail(YCGE_ERR_UNSUPPORTED, "voxel storage exceeds 4 GiB");
            pl.off = (uint32_t)off;
            P.arena_end = off + pl.cap;
        }
        if (!P.free_luts.empty()) { pl.lut = P.free_luts.back(); P.free_luts.pop_back(); }
        else {
            if (P.lut_end + YCGE_ENC_LUT_ENTRIES >= ((uint64_t)1 << 32)) return c->fail(YCGE_ERR_UNSUPPORTED, "voxel material tables exceed 2^32 entries");
            pl.lut = (uint32_t)P.lut_end; P.lut_end += YCGE_ENC_LUT_ENTRIES;
        }
        pl.direct = (size_t)pl.off + pl.cap <= arena_cap;
        if (pl.device && !pl.direct) { pl.scratch_off = scratch; scratch = align_up(scratch + pl.cap, 256); }
        const size_t i = (size_t)pl.index;
        P.resident[i] = 1; P.block_bytes[i] = pl.cap; P.lut_region[i] = (int32_t)pl.lut;
        P.arena_in_use += pl.cap; P.n_resident++;
        pl.rec.cell_offset = pl.off; pl.rec.lut_offset = pl.lut;
    }
    if (P.owner.size() < P.recs.size()) P.owner.resize(P.recs.size(), -1);

    // ---- room for the tables (contents kept; the arena waits for the verdicts)
    std::vector<ycge_ctx *> ctxs{c};
    ctxs.insert(ctxs.end(), c->peers.begin(), c->peers.end());
    for (ycge_ctx *x : ctxs) {
        HIP_TRY(c, hipSetDevice(x->device));
        const size_t lut_have = x->d_lut.p ? x->d_lut.cap : 0, grids_have = x->d_grids.p ? x->d_grids.cap : 0;
        if (P.lut_end > lut_have) {
            const hipError_t e = grow_preserve(x->d_lut, std::max<size_t>((size_t)P.lut_end, 2 * lut_have), x->d_lut.p ? x->d_lut.n : 0);
            x->sd.grid_lut = x->d_lut.p;
            HIP_TRY(c, e);
        }
        if (P.recs.size() > grids_have) {
            const hipError_t e = grow_preserve(x->d_grids, std::max<size_t>(P.recs.size(), 2 * grids_have), x->d_grids.p ? x->d_grids.n : 0);
            x->sd.grids = x->d_grids.p;
            HIP_TRY(c, e);
        }
        if (scratch > x->d_enc_out.cap) HIP_TRY(c, x->d_enc_out.alloc(scratch));
    }
    HIP_TRY(c, hipSetDevice(c->device));

    // ---- the device encoder, in groups of at most 256 MiB of raw cells (a larger grid is a group of its own)
    std::vector<GridEncResult> res((size_t)n);
    double us[4] = {0, 0, 0, 0};
    {
        std::vector<int> group;
        size_t group_bytes = 0;
        const size_t budget = c->knobs.enc_group_bytes;          // (256 MiB; YCGE_ENC_GROUP_BYTES)
        for (int k = 0; k <= n; k++) {
            const size_t bytes = k < n ? (size_t)grids[k].nx * grids[k].ny * grids[k].nz * 8 : 0;
            if (!group.empty() && (k == n || group_bytes + bytes > budget)) {
                rc = encode_group(c, grids, plan, group, res, us, gen);
                if (rc != YCGE_OK) return rc;
                group.clear(); group_bytes = 0;
            }
            if (k < n && plan[(size_t)k].device) { group.push_back(k); group_bytes += bytes; }
            if (gen && group.size() >= kGenGroupMax) group_bytes = budget;          // (a full fill launch: the next grid opens a new group)
        }
    }
    // ---- verdicts, records, the host encoder for the rest
    for (int k = 0; k < n; k++) {
        Planned &pl = plan[(size_t)k];
        const ycge_grid &g = grids[k];
        int lo[3], hi[3];
        uint64_t mask = 0;
        if (pl.device) {
            const GridEncResult &r = res[(size_t)k];
            if (r.bad_cell != 0xffffffffu)          // (generated grids: encode_group has named it already)
                return c->fail(YCGE_ERR_INVALID_ARG, "grid %d: no material for (matId %d, metaId %d)", k, g.cells[2 * (size_t)r.bad_cell], g.cells[2 * (size_t)r.bad_cell + 1]);
            // (the generator writes a dozen distinct pairs at most: never asked for its grids)
            if (!gen && r.any_miss && too_many_pairs(g)) return c->fail(YCGE_ERR_UNSUPPORTED, "grid %d: more than 255 distinct (matId, metaId) pairs", k);
            for (int a = 0; a < 3; a++) { lo[a] = r.lo[a]; hi[a] = r.hi[a]; }
            mask = pl.rec.has_brick_mask ? ((uint64_t)r.mask_hi << 32) | r.mask_lo : 0;
            P.device_encodes++;
        } else {
            pl.host_bytes.assign(pl.cap, 0);
            ycge_grid gh = g;
            std::vector<int32_t> made;
            if (gen && gen->world) {          // (ycge_scene_generate_world takes the host generator for such a table: the world is there)
                made.resize(gen->chunk_bytes() / 4);
                world_slice(*gen, gen->keys[(size_t)k], gen->host_world, made.data());
                gh.cells = made.data();
            } else if (gen) {          // a lookup table too large for k_grid_encode: this chunk's cells are made here, whoever makes the others
                std::vector<wg::ColRec> cols((size_t)gen->W.size * gen->W.size);
                int32_t any = 0;
                made.resize(gen->chunk_bytes() / 4);
                worldgen_columns_host(gen->W, gen->keys[(size_t)k][0], gen->keys[(size_t)k][2], cols.data());
                worldgen_fill_host(gen->W, cols.data(), gen->keys[(size_t)k][0], gen->keys[(size_t)k][1], gen->keys[(size_t)k][2], made.data(), &any);
                if (!gen->cells_out.empty()) std::memcpy(gen->cells_out[(size_t)k], made.data(), gen->chunk_bytes());
                gh.cells = made.data();
            }
            rc = encode_grid_host(c, gh, k, c->n_materials, pl.rec, pl.host_bytes.data(), pl.host_lut, lo, hi, mask);
            if (rc != YCGE_OK) return rc;
            pl.host_lut.resize(YCGE_ENC_LUT_ENTRIES, -1);
            P.host_encodes++;
        }
        grid_record_solid(pl.rec, lo, hi, mask);
        const size_t i = (size_t)pl.index;
        P.recs[i] = pl.rec;
        bounds[i] = grid_world_bounds(g);
        for (int a = 0; a < 3; a++) { solid[i][a] = pl.rec.solid_lo[a]; solid[i][3 + a] = pl.rec.solid_hi[a]; }
        solid[i][6] = pl.rec.cull_t_limit;
    }
    // ---- every verdict is in: the arena grows (geometrically) where the plan runs past it, the waiting bytes move in, the table goes up
    const bool grow = P.arena_end > arena_cap;
    if (grow) {
        // the larger arenas of ALL devices are made (and filled with the resident bytes) before any device takes its own: an allocation
        // that fails on one of them leaves every device's capacity as it was
        P.growths++;
        const size_t want = std::min<size_t>(std::max<size_t>((size_t)P.arena_end, 2 * arena_cap), ((size_t)1 << 32) - 1);
        std::vector<DevBuf<uint8_t>> larger(ctxs.size());
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < ctxs.size() && e == hipSuccess; i++) {
            ycge_ctx *x = ctxs[i];
            e = hipSetDevice(x->device);
            if (e == hipSuccess) e = larger[i].alloc(want);
            if (e == hipSuccess && x->d_cells.p && x->d_cells.n) e = hipMemcpy(larger[i].p, x->d_cells.p, x->d_cells.n, hipMemcpyDeviceToDevice);
        }
        if (e != hipSuccess) (void)hipSetDevice(c->device);          // (the larger arenas made so far go with `larger`: a free takes any device's memory, whichever is current)
        HIP_TRY(c, e);
        for (size_t i = 0; i < ctxs.size(); i++) {
            ycge_ctx *x = ctxs[i];
            (void)hipSetDevice(x->device);
            const size_t used = x->d_cells.n;
            x->d_cells = std::move(larger[i]);
            x->d_cells.n = used;
            x->sd.grid_cells = x->d_cells.p;
        }
    }
    for (ycge_ctx *x : ctxs) {
        HIP_TRY(c, hipSetDevice(x->device));
        for (int k = 0; k < n; k++) {
            const Planned &pl = plan[(size_t)k];
            if (pl.device && !pl.direct) HIP_TRY(c, hipMemcpyAsync(x->d_cells.p + pl.off, x->d_enc_out.p + pl.scratch_off, pl.cap, hipMemcpyDeviceToDevice, x->stream));
            if (!pl.device) {
                HIP_TRY(c, hipMemcpy(x->d_cells.p + pl.off, pl.host_bytes.data(), pl.cap, hipMemcpyHostToDevice));
                HIP_TRY(c, hipMemcpy(x->d_lut.p + pl.lut, pl.host_lut.data(), YCGE_ENC_LUT_ENTRIES * sizeof(int32_t), hipMemcpyHostToDevice));
            }
        }
        HIP_TRY(c, hipMemcpy(x->d_grids.p, P.recs.data(), P.recs.size() * sizeof(GGrid), hipMemcpyHostToDevice));
        HIP_TRY(c, hipStreamSynchronize(x->stream));
        x->d_grids.n = P.recs.size();
        if (x->d_cells.n < (size_t)P.arena_end) x->d_cells.n = (size_t)P.arena_end;
        if (x->d_lut.n < (size_t)P.lut_end) x->d_lut.n = (size_t)P.lut_end;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    for (int a = 0; a < 4; a++) P.last_attach_us[a] = us[a];
    P.streamed = true;
    // ---- nothing below fails
    c->grid_pool = std::move(P);
    c->grid_bounds.swap(bounds);
    c->grid_solid.swap(solid);
    for (int k = 0; k < n; k++) out_grid_index[k] = plan[(size_t)k].index;
    return query_scene_changed(c);
}

int ycge_scene_attach_grids(ycge_ctx *c, const ycge_grid *grids, int32_t n, int32_t *out_grid_index)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0 || (n > 0 && (!grids || !out_grid_index))) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_attach_grids: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    for (int k = 0; k < n; k++) {
        std::string m;
        const int vrc = validate_grid(grids[k], k, c->n_materials, m);
        if (vrc != YCGE_OK) return c->fail(vrc, "%s", m.c_str());
    }
    return attach_common(c, grids, n, out_grid_index, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

// ycge_scene_generate_grids: the chunk columns first (every 2-D field of WorldGenerator.GenerateChunkCells, once per distinct (cx, cz)) -
// their tops say which chunks hold anything, and only those take part in the attach; then attach_common with a GenSource, whose groups are
// the sub-batches.  Everything before attach_common changes scratch buffers only, and attach_common is all or nothing.
int ycge_scene_generate_grids(ycge_ctx *c, const ycge_world *world, const int32_t *keys, int32_t n, const ycge_grid *proto, int32_t *out_grid_index, int32_t *cells_out)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    const char *why = nullptr;
    if (worldgen_check(world, &why) != YCGE_OK) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_grids: %s", why);
    if (n < 0 || (n > 0 && (!keys || !out_grid_index)) || !proto) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_grids: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    const int S = world->chunk_size;
    static const int32_t no_cells[2] = {0, 0};          // (validate_grid wants a pointer; a generated grid's cells are never read through it)
    ycge_grid g0 = *proto;
    g0.nx = g0.ny = g0.nz = S; g0.voxel_size = world->voxel_size; g0.cells = no_cells;
    {
        std::string m;
        const int vrc = validate_grid(g0, 0, c->n_materials, m);
        if (vrc != YCGE_OK) return c->fail(vrc, "%s", m.c_str());
    }
    for (int k = 0; k < n; k++)
        if (worldgen_key_check(world, keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]) != YCGE_OK)          // (block coordinates stay exact in binary32, as the generator assumes)
            return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_grids: key %d is outside +-2^24 blocks", k);
    int rc = quiesce(c);
    for (ycge_ctx *p : c->peers) if (rc == YCGE_OK) rc = quiesce(p);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const DeviceGuard guard(c->device);

    GenSource all;          // every key; `gen` below keeps the ones that hold something
    all.W = wg::make_world(S, world->chunks_y, world->world_seed);
    all.host = c->knobs.worldgen_host;
    const size_t S2 = (size_t)S * S, chunk_i32 = 2 * S2 * S;
    std::vector<std::array<int32_t, 2>> col_keys;
    {
        std::map<std::pair<int32_t, int32_t>, int32_t> seen;
        for (int k = 0; k < n; k++) {
            const auto ins = seen.insert({{keys[3 * k], keys[3 * k + 2]}, (int32_t)col_keys.size()});
            if (ins.second) col_keys.push_back({{keys[3 * k], keys[3 * k + 2]}});
            all.keys.push_back({{keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]}});
            all.col.push_back(ins.first->second);
        }
    }
    const size_t n_cols = col_keys.size();
    std::vector<int32_t> col_top(n_cols);
    c->worldgen_last_us[0] = c->worldgen_last_us[1] = 0;
    std::vector<ycge_ctx *> ctxs{c};
    ctxs.insert(ctxs.end(), c->peers.begin(), c->peers.end());
    const size_t cols_bytes = align_up(n_cols * S2 * sizeof(wg::ColRec), 256), keys_bytes = align_up(n_cols * 8, 256);
    if (all.host) {
        all.host_cols.resize(n_cols * S2);
        for (size_t j = 0; j < n_cols; j++) {
            worldgen_columns_host(all.W, col_keys[j][0], col_keys[j][1], all.host_cols.data() + j * S2);
            int32_t top = INT32_MIN;
            for (size_t i = 0; i < S2; i++) { const wg::ColRec &R = all.host_cols[j * S2 + i]; top = std::max(top, std::max(R.ground, R.water)); }
            col_top[j] = top;
        }
    } else {
        for (ycge_ctx *x : ctxs) {
            HIP_TRY(c, hipSetDevice(x->device));
            const size_t need = cols_bytes + keys_bytes + n_cols * 4;
            if (x->d_wg_cols.cap < need) HIP_TRY(c, x->d_wg_cols.alloc(need));
            uint8_t *d_keys = x->d_wg_cols.p + cols_bytes, *d_top = d_keys + keys_bytes;
            const auto t0 = std::chrono::steady_clock::now();
            HIP_TRY(c, hipMemcpyAsync(d_keys, col_keys.data(), n_cols * 8, hipMemcpyHostToDevice, x->stream));
            const int e = ycge_launch_worldgen_columns((const int32_t *)d_keys, (int)n_cols, &all.W, (wg::ColRec *)x->d_wg_cols.p, (int32_t *)d_top, x->stream);
            if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wg_columns launch failed: %s", hipGetErrorString((hipError_t)e));
            HIP_TRY(c, hipStreamSynchronize(x->stream));
            if (x == c) {
                c->worldgen_last_us[0] = us_since(t0);
                rc = copy_out(c, col_top.data(), d_top, n_cols * 4);
                if (rc != YCGE_OK) return rc;
            }
        }
        HIP_TRY(c, hipSetDevice(c->device));
    }
    // a chunk holds something exactly when a column reaches into or above it: Water up to localWater, ground below (trees stand on ground of their own chunk)
    GenSource gen;
    gen.W = all.W; gen.host = all.host; gen.host_cols.swap(all.host_cols);
    std::vector<int> solid_k, air_k;
    for (int k = 0; k < n; k++) (col_top[(size_t)all.col[(size_t)k]] >= all.keys[(size_t)k][1] * S ? solid_k : air_k).push_back(k);
    std::vector<ycge_grid> grids;
    for (int k : solid_k) {
        ycge_grid g = g0;
        const auto &key = all.keys[(size_t)k];
        g.min_corner.x = world->world_min.x + (float)(key[0] * S) * world->voxel_size.x;          // WorldManager.cs:761-768
        g.min_corner.y = world->world_min.y + (float)(key[1] * S) * world->voxel_size.y;
        g.min_corner.z = world->world_min.z + (float)(key[2] * S) * world->voxel_size.z;
        grids.push_back(g);
        gen.keys.push_back(key); gen.col.push_back(all.col[(size_t)k]);
        if (cells_out) gen.cells_out.push_back(cells_out + (size_t)k * chunk_i32);
    }
    // the empty chunks' cells, when asked for: made like the others (and found empty), in launches of their own
    if (cells_out && !air_k.empty()) {
        if (gen.host) {
            for (int k : air_k) {
                int32_t any = 0;
                const auto &key = all.keys[(size_t)k];
                worldgen_fill_host(gen.W, gen.host_cols.data() + (size_t)all.col[(size_t)k] * S2, key[0], key[1], key[2], cells_out + (size_t)k * chunk_i32, &any);
                if (any) return c->fail(YCGE_ERR_INTERNAL, "ycge_scene_generate_grids: chunk (%d, %d, %d) holds cells above its column's top", key[0], key[1], key[2]);
            }
        } else {
            const size_t slot = align_up(chunk_i32 * 4, 256), per = std::max<size_t>(1, std::min<size_t>(kGenGroupMax, ((size_t)64 << 20) / slot));
            for (size_t first = 0; first < air_k.size(); first += per) {
                const size_t m = std::min(per, air_k.size() - first);
                const size_t off_any = align_up(m * sizeof(WgChunk), 256), off_cells = align_up(off_any + m * 4, 256), total = off_cells + m * slot;
                if (c->d_enc_in.cap < total) HIP_TRY(c, c->d_enc_in.alloc(total));
                std::vector<uint8_t> head(off_cells, 0);
                for (size_t j = 0; j < m; j++) {
                    const int k = air_k[first + j];
                    WgChunk w;
                    w.cx = all.keys[(size_t)k][0]; w.cy = all.keys[(size_t)k][1]; w.cz = all.keys[(size_t)k][2]; w.col = all.col[(size_t)k];
                    w.cells = (int32_t *)(c->d_enc_in.p + off_cells + j * slot);
                    std::memcpy(head.data() + j * sizeof(WgChunk), &w, sizeof w);
                }
                HIP_TRY(c, hipMemcpy(c->d_enc_in.p, head.data(), off_cells, hipMemcpyHostToDevice));
                const int e = ycge_launch_worldgen_fill((const WgChunk *)c->d_enc_in.p, (int)m, &gen.W, (const wg::ColRec *)c->d_wg_cols.p, (uint32_t *)(c->d_enc_in.p + off_any), c->stream);
                if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wg_fill launch failed: %s", hipGetErrorString((hipError_t)e));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                std::vector<uint32_t> any(m);
                rc = copy_out(c, any.data(), c->d_enc_in.p + off_any, m * 4);
                for (size_t j = 0; j < m && rc == YCGE_OK; j++) {
                    const int k = air_k[first + j];
                    if (any[j]) return c->fail(YCGE_ERR_INTERNAL, "ycge_scene_generate_grids: chunk (%d, %d, %d) holds cells above its column's top", all.keys[(size_t)k][0], all.keys[(size_t)k][1], all.keys[(size_t)k][2]);
                    rc = copy_out(c, cells_out + (size_t)k * chunk_i32, c->d_enc_in.p + off_cells + j * slot, chunk_i32 * 4);
                }
                if (rc != YCGE_OK) return rc;
            }
        }
    }
    std::vector<int32_t> idx(solid_k.size(), -1);
    if (!solid_k.empty()) {
        rc = attach_common(c, grids.data(), (int32_t)grids.size(), idx.data(), &gen);
        if (rc != YCGE_OK) return rc;
    }
    {          // who made the cells: the kernels, or the host generator (the knob; a lookup table too large for k_grid_encode).  An empty chunk's cells are made only when cells_out asks.
        const bool solid_on_host = gen.host || proto->n_lookup > YCGE_ENC_MAX_LOOKUP;
        const int64_t n_air = cells_out ? (int64_t)air_k.size() : 0, n_solid = (int64_t)solid_k.size();
        c->worldgen_host_chunks += (solid_on_host ? n_solid : 0) + (gen.host ? n_air : 0);
        c->worldgen_device_chunks += (solid_on_host ? 0 : n_solid) + (gen.host ? 0 : n_air);
    }
    for (int k : air_k) out_grid_index[k] = -1;
    for (size_t j = 0; j < solid_k.size(); j++) out_grid_index[solid_k[j]] = idx[j];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// ycge_scene_generate_world: the 2-D fields of the window first (on every device), the anyLeaves flags to their fixed point, then one
// word per chunk - does it hold anything (AttachChunkFromPreloaded, WorldManager.cs:704-720: any cell not Air, trees from other chunks
// included; EXACT, chunk by chunk: between a column's ground and a neighbour's canopy above it a whole small chunk can be Air) - then attach_common with a GenSource of the chunks that do, whose groups are the sub-batches k_wp_fill fills.  Everything
// before attach_common changes scratch buffers only, and attach_common is all or nothing.
int ycge_scene_generate_world(ycge_ctx *c, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, const ycge_grid *proto,
                              int32_t *out_grid_index, int32_t *cells_out)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    const char *why = nullptr;
    if (worldgen_check(world, &why) != YCGE_OK || worldgen_window_check(world, chunks_x, chunks_z, origin_bx, origin_bz, &why) != YCGE_OK)
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_world: %s", why);
    if (!out_grid_index || !proto) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_generate_world: null argument");
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    const int S = world->chunk_size, chunks_y = world->chunks_y;
    static const int32_t no_cells[2] = {0, 0};
    ycge_grid g0 = *proto;
    g0.nx = g0.ny = g0.nz = S; g0.voxel_size = world->voxel_size; g0.cells = no_cells;
    {
        std::string m;
        const int vrc = validate_grid(g0, 0, c->n_materials, m);
        if (vrc != YCGE_OK) return c->fail(vrc, "%s", m.c_str());
    }
    int rc = quiesce(c);
    for (ycge_ctx *p : c->peers) if (rc == YCGE_OK) rc = quiesce(p);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const DeviceGuard guard(c->device);

    GenSource gen;
    gen.world = true;
    gen.W = wg::make_world(S, chunks_y, world->world_seed);
    gen.N = wg::Window{chunks_x * S, chunks_z * S, origin_bx, origin_bz};
    gen.host = c->knobs.worldgen_host || proto->n_lookup > YCGE_ENC_MAX_LOOKUP;          // (a table k_grid_encode does not take: every chunk is encoded on the host, from the host's cells)
    const size_t n_cols = (size_t)gen.N.nx * gen.N.nz, ny = (size_t)gen.W.height, n_chunks = (size_t)chunks_x * chunks_y * chunks_z;
    const size_t world_i32 = 2 * n_cols * ny;
    std::vector<uint8_t> occupied(n_chunks, 0);          // per chunk, (cx, cy, cz) with cx outermost
    std::vector<int32_t> host_world;
    for (double &u : c->worldpregen_last_us) u = 0;
    c->worldpregen_last_passes = 0;
    if (gen.host) {
        int32_t *w = cells_out;
        if (!w) { host_world.resize(world_i32); w = host_world.data(); }
        world_cells_host(world, chunks_x, chunks_z, origin_bx, origin_bz, w);
        gen.host_world = w;
        for (size_t x = 0; x < (size_t)gen.N.nx; x++)
            for (size_t y = 0; y < ny; y++) {
                const int32_t *row = w + 2 * ((x * ny + y) * gen.N.nz);
                for (size_t z = 0; z < (size_t)gen.N.nz; z++)
                    if (row[2 * z] != 0) occupied[((x / S) * chunks_y + y / S) * chunks_z + z / S] = 1;
            }
    } else {
        std::vector<ycge_ctx *> ctxs{c};
        ctxs.insert(ctxs.end(), c->peers.begin(), c->peers.end());
        std::vector<uint32_t> occ_words(n_chunks);
        int root_passes = 0;
        for (ycge_ctx *x : ctxs) {          // (the root first: a peer repeats its passes without reading anything back)
            HIP_TRY(c, hipSetDevice(x->device));
            const size_t need = wp_layout(nullptr, n_cols, n_chunks, nullptr);
            if (x->d_wg_cols.cap < need) HIP_TRY(c, x->d_wg_cols.alloc(need));
            WpFields F;
            wp_layout(x->d_wg_cols.p, n_cols, n_chunks, &F);
            uint8_t *flags[2] = {F.fallback, wp_next_flags(F, n_cols)};
            auto t0 = std::chrono::steady_clock::now();
            int e = ycge_launch_worldpregen_fields(&gen.W, &gen.N, &F, x->stream);
            if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_* launch failed: %s", hipGetErrorString((hipError_t)e));
            HIP_TRY(c, hipStreamSynchronize(x->stream));
            if (x == c) c->worldpregen_last_us[0] = us_since(t0);
            t0 = std::chrono::steady_clock::now();
            int passes = 0, cur = 0;
            for (;;) {          // anyLeaves: from flags[cur] into flags[1 - cur] until a pass flips nothing (then both hold the fixed point)
                F.fallback = flags[cur];
                e = ycge_launch_worldpregen_any_leaves(&gen.W, &gen.N, &F, flags[1 - cur], x->stream);
                if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_any_leaves launch failed: %s", hipGetErrorString((hipError_t)e));
                passes++;
                if (x != c) { if (passes == root_passes) break; cur = 1 - cur; continue; }
                HIP_TRY(c, hipStreamSynchronize(x->stream));
                uint32_t changed = 0;
                rc = copy_out(c, &changed, F.changed, sizeof changed);
                if (rc != YCGE_OK) return rc;
                if (!changed) break;
                if ((size_t)passes > n_cols + 1) return c->fail(YCGE_ERR_INTERNAL, "ycge_scene_generate_world: the anyLeaves passes do not settle");
                cur = 1 - cur;
            }
            F.fallback = flags[0];          // (the last pass flipped nothing: both buffers hold the fixed point, and wp_layout names this one)
            if (x == c) { root_passes = c->worldpregen_last_passes = passes; c->worldpregen_last_us[1] = us_since(t0); }
            t0 = std::chrono::steady_clock::now();
            if (x == c) {
                e = ycge_launch_worldpregen_occupied(&gen.W, &gen.N, &F, chunks_y, chunks_z, n_chunks, x->stream);
                if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_occupied launch failed: %s", hipGetErrorString((hipError_t)e));
            }
            HIP_TRY(c, hipStreamSynchronize(x->stream));
            if (x == c) {
                rc = copy_out(c, occ_words.data(), F.occupied, n_chunks * 4);
                if (rc != YCGE_OK) return rc;
                c->worldpregen_last_us[2] = us_since(t0);
            }
        }
        HIP_TRY(c, hipSetDevice(c->device));
        for (size_t k = 0; k < n_chunks; k++) occupied[k] = occ_words[k] != 0;
        if (cells_out) { std::memset(cells_out, 0, world_i32 * 4); gen.world_out = cells_out; }          // (a chunk that holds nothing is (Air, 0) throughout)
    }
    std::vector<ycge_grid> grids;
    std::vector<size_t> solid_k;
    for (int cx = 0; cx < chunks_x; cx++)
        for (int cy = 0; cy < chunks_y; cy++)
            for (int cz = 0; cz < chunks_z; cz++) {
                const size_t k = ((size_t)cx * chunks_y + cy) * chunks_z + cz;
                if (!occupied[k]) continue;
                ycge_grid g = g0;
                g.min_corner.x = world->world_min.x + (float)(cx * S) * world->voxel_size.x;          // WorldManager.cs:722-726
                g.min_corner.y = world->world_min.y + (float)(cy * S) * world->voxel_size.y;
                g.min_corner.z = world->world_min.z + (float)(cz * S) * world->voxel_size.z;
                grids.push_back(g);
                gen.keys.push_back({{cx, cy, cz}}); gen.col.push_back(0);
                solid_k.push_back(k);
            }
    std::vector<int32_t> idx(solid_k.size(), -1);
    if (!solid_k.empty()) {
        c->worldgen_last_us[1] = 0;
        rc = attach_common(c, grids.data(), (int32_t)grids.size(), idx.data(), &gen);
        if (rc != YCGE_OK) return rc;
        c->worldpregen_last_us[3] = c->worldgen_last_us[1];
    }
    (gen.host ? c->worldgen_host_chunks : c->worldgen_device_chunks) += (int64_t)n_chunks;
    for (size_t k = 0; k < n_chunks; k++) out_grid_index[k] = -1;
    for (size_t j = 0; j < solid_k.size(); j++) out_grid_index[solid_k[j]] = idx[j];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: the last ycge_scene_generate_world on the root device - {anyLeaves passes (the last flips nothing), us of the
// 2-D field kernels, of the anyLeaves pass loop (WALL time: each pass is a launch, a stream synchronise and a 4-byte read-back), of the
// occupancy kernel and its read-back, of the fill kernels}
int ycge_debug_worldpregen_stats(ycge_ctx *c, int64_t *out5)
try {
    if (!c || !out5) return YCGE_ERR_INVALID_ARG;
    out5[0] = c->worldpregen_last_passes;
    for (int a = 0; a < 4; a++) out5[1 + a] = (int64_t)c->worldpregen_last_us[a];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: {chunks made on the device, chunks made on the host, the last call's column kernel and fill + tree kernels in microseconds (root device)}
int ycge_debug_worldgen_stats(ycge_ctx *c, int64_t *out4)
try {
    if (!c || !out4) return YCGE_ERR_INVALID_ARG;
    out4[0] = c->worldgen_device_chunks; out4[1] = c->worldgen_host_chunks; out4[2] = (int64_t)c->worldgen_last_us[0]; out4[3] = (int64_t)c->worldgen_last_us[1];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_scene_detach_grids(ycge_ctx *c, const int32_t *grid_index, int32_t n)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0 || (n > 0 && !grid_index)) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_grids: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return YCGE_OK;
    GridPool P = c->grid_pool;
    std::vector<std::array<float, 6>> bounds = c->grid_bounds;
    std::vector<std::array<float, 7>> solid = c->grid_solid;
    for (int k = 0; k < n; k++) {
        const int32_t gi = grid_index[k];
        if (gi < 0 || (size_t)gi >= c->grid_pool.recs.size() || !c->grid_pool.resident[(size_t)gi])
            return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_grids: grid %d is not resident", gi);
        if (!P.resident[(size_t)gi]) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_grids: grid %d is named twice", gi);
        if ((size_t)gi < P.owner.size() && P.owner[(size_t)gi] >= 0)
            return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_detach_grids: grid %d is held by object %d of Scene.Objects", gi, P.owner[(size_t)gi]);
        const size_t i = (size_t)gi;
        P.resident[i] = 0;
        P.free_index.insert(gi);
        P.free_blocks.insert({P.block_bytes[i], P.recs[i].cell_offset});
        if (P.lut_region[i] >= 0) P.free_luts.push_back((uint32_t)P.lut_region[i]);
        P.arena_in_use -= P.block_bytes[i]; P.n_resident--;
        P.block_bytes[i] = 0; P.lut_region[i] = -1;
        std::memset(&P.recs[i], 0, sizeof(GGrid));
        bounds[i] = std::array<float, 6>{{0, 0, 0, -1, -1, -1}};
        solid[i] = std::array<float, 7>{};
    }
    while (!P.recs.empty() && !P.resident.back()) {          // the tables follow the resident set: free slots at the end go
        P.free_index.erase((int32_t)P.recs.size() - 1);
        P.recs.pop_back(); P.resident.pop_back(); P.block_bytes.pop_back(); P.lut_region.pop_back();
        bounds.pop_back(); solid.pop_back();
    }
    if (P.owner.size() > P.recs.size()) P.owner.resize(P.recs.size());
    P.streamed = true;
    c->grid_pool = std::move(P);
    c->grid_bounds.swap(bounds);
    c->grid_solid.swap(solid);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: grid `grid_index` as the device holds it - its record (sizeof GGrid bytes) and, per voxel in ycge_grid.cells order, the
// material its cell code stands for (-1: empty)
int ycge_debug_read_grid(ycge_ctx *c, int32_t grid_index, void *record_out, int32_t *materials_out)
try {
    if (!c || !c->have_scene || !record_out || !materials_out) return YCGE_ERR_INVALID_ARG;
    const GridPool &P = c->grid_pool;
    if (grid_index < 0 || (size_t)grid_index >= P.recs.size() || !P.resident[(size_t)grid_index]) return c->fail(YCGE_ERR_INVALID_ARG, "grid %d is not resident", grid_index);
    int rc = quiesce(c);
    if (rc != YCGE_OK) return rc;
    GGrid G;
    rc = copy_out(c, &G, c->d_grids.p + grid_index, sizeof G);
    if (rc != YCGE_OK) return rc;
    std::memcpy(record_out, &G, sizeof G);
    const size_t cap = (size_t)G.nbx * G.nby * G.nbz * 512;
    if ((size_t)G.cell_offset + cap > c->d_cells.n || G.lut_offset >= c->d_lut.n) return c->fail(YCGE_ERR_INTERNAL, "grid %d: record out of range", grid_index);
    std::vector<uint8_t> bytes(cap);
    std::vector<int32_t> lut(std::min<size_t>(256, c->d_lut.n - G.lut_offset));
    rc = copy_out(c, bytes.data(), c->d_cells.p + G.cell_offset, cap);
    if (rc == YCGE_OK) rc = copy_out(c, lut.data(), c->d_lut.p + G.lut_offset, lut.size() * sizeof(int32_t));
    if (rc != YCGE_OK) return rc;
    for (int ix = 0; ix < G.nx; ix++)
        for (int iy = 0; iy < G.ny; iy++)
            for (int iz = 0; iz < G.nz; iz++) {
                const int brick = (((iz >> 3) * G.nby) + (iy >> 3)) * G.nbx + (ix >> 3);
                const uint8_t code = bytes[(size_t)brick * 512 + morton3_host(ix & 7, iy & 7, iz & 7)];
                materials_out[((size_t)ix * G.ny + iy) * G.nz + iz] = code == 0 ? -1 : ((size_t)code < lut.size() ? lut[code] : -2);
            }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the context that drives device k + 1 of a one-process multi-device context (NULL: none) - what a caller must NOT hand to the scene calls
ycge_ctx *ycge_debug_peer_context(ycge_ctx *c, int32_t k)
try {
    return (c && k >= 0 && (size_t)k < c->peers.size()) ? c->peers[(size_t)k] : nullptr;
}
catch (...) { (void)ycge_host::abi_catch(c); return nullptr; }

// test / profiling hook: {resident grids, free indices, arena bytes in use, arena capacity, arena growths, slots reused, device encodes,
// host-fallback encodes, then the last attach in microseconds: copy into the staging, host-to-device copy, encode kernel, read-back}
int ycge_debug_grid_pool_stats(ycge_ctx *c, int64_t *out12)
try {
    if (!c || !out12) return YCGE_ERR_INVALID_ARG;
    const GridPool &P = c->grid_pool;
    out12[0] = P.n_resident; out12[1] = (int64_t)P.free_index.size(); out12[2] = (int64_t)P.arena_in_use;
    out12[3] = (int64_t)(c->d_cells.p ? c->d_cells.cap : 0); out12[4] = P.growths; out12[5] = P.slots_reused;
    out12[6] = P.device_encodes; out12[7] = P.host_encodes;
    for (int a = 0; a < 4; a++) out12[8 + a] = (int64_t)P.last_attach_us[a];
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
