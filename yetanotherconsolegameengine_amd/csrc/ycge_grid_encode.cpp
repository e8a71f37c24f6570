// ycge_grid_encode.cpp - chunk streaming: ycge_scene_attach_grids / ycge_scene_detach_grids and the pool of resident voxel grids.
//
// The reference's voxel world attaches and removes VolumeGrids every frame (VolumeScene.Update -> WorldManager.LoadChunksAround,
// Scenes/VolumeScenes.cs:63-64, WorldManager.cs:289-370).  An attach brings the raw cells of its grids up once through page-locked
// staging; k_grid_encode (ycge_grid_encode.hip) writes the bricked bytes, the solid box, the brick mask and the "no material" verdict of
// the whole batch in one launch, and one small read-back tells the host what flatten_objects needs.  Grids whose lookup table exceeds
// YCGE_ENC_MAX_LOOKUP entries take the host encoder of ycge_scene_upload.  Where the raw cells come from is a CellSource's business (ycge_ctx.h): the caller's here.
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
#include <unordered_set>

#include "ycge_ctx.h"
#include "ycge_grid_encode.h"

namespace ycge_host {

void grid_pool_reset(ycge_ctx *c, const std::vector<GGrid> &recs, size_t arena_bytes, size_t lut_entries, std::vector<SlotCodes> codes)
{
    GridPool P;
    const size_t n = recs.size();
    P.recs = recs;
    P.codes = std::move(codes);
    P.codes.resize(n);
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

int morton3_host(int x, int y, int z)
{
    return ((x & 1) << 0) | ((y & 1) << 1) | ((z & 1) << 2) | ((x & 2) << 2) | ((y & 2) << 3) | ((z & 2) << 4) | ((x & 4) << 4) | ((y & 4) << 5) | ((z & 4) << 6);
}

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

// ycge_scene_attach_grids: the caller brought the cells
struct CallerCells : CellSource {
    CallerCells() { caller_cells = true; }
    int write(ycge_ctx *, size_t, const ycge_grid &g, int32_t *cells) override { std::memcpy(cells, g.cells, (size_t)g.nx * g.ny * g.nz * 8); return YCGE_OK; }
};

// one group of device-encoded grids: stage, copy, (fill,) launch, read back (every device of the context; the root's results are returned)
int encode_group(ycge_ctx *root, const ycge_grid *grids, std::vector<Planned> &plan, const std::vector<int> &group, std::vector<GridEncResult> &res, double us[4], CellSource &src)
{
    const DeviceGuard guard(root->device);
    const size_t m = group.size();
    size_t at = align_up(m * sizeof(GridEncDesc), 256);
    const size_t off_res = at;
    at = align_up(at + m * sizeof(GridEncResult), 256);
    const size_t off_head = at;
    at = align_up(at + src.head_bytes(m), 256);
    for (int k : group) { plan[k].lookup_off = at; at = align_up(at + (size_t)grids[k].n_lookup * sizeof(ycge_voxel_lookup), 16); }
    at = align_up(at, 256);
    const size_t off_cells = at;
    for (int k : group) { plan[k].cells_off = at; at = align_up(at + (size_t)grids[k].nx * grids[k].ny * grids[k].nz * 8, 256); }
    const size_t dev_total = at;                                                    // what the device holds
    const size_t up_bytes = src.on_device ? off_cells : at, off_back = up_bytes;    // what goes up; where the results come back to (staging only)
    HIP_TRY(root, root->enc_stage.reserve(off_back + m * sizeof(GridEncResult), hipHostMallocPortable));      // (every device of the context copies from it)
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
        const int rc = src.on_device ? YCGE_OK : src.write(root, (size_t)group[j], g, (int32_t *)(st + pl.cells_off));
        if (rc != YCGE_OK) return rc;
        first_wg[j] = n_wg;
        const uint64_t wgs = (uint64_t)pl.rec.nbx * pl.rec.nby * (((uint64_t)pl.rec.nbz + YCGE_ENC_RUN - 1) / YCGE_ENC_RUN);
        if (n_wg + wgs >= 0x7fffffffull) return root->fail(YCGE_ERR_UNSUPPORTED, "ycge_scene_attach_grids: more bricks in one batch than one launch takes");
        n_wg += (uint32_t)wgs;
    }
    us[0] += us_since(t0);
    std::vector<int32_t *> d_cells(m);
    for (ycge_ctx *c : contexts_of(root)) {
        HIP_TRY(root, hipSetDevice(c->device));
        if (c->d_enc_in.cap < dev_total) HIP_TRY(root, c->d_enc_in.alloc(dev_total));
        GridEncDesc *descs = (GridEncDesc *)st;
        for (size_t j = 0; j < m; j++) {
            const ycge_grid &g = grids[group[j]];
            const Planned &pl = plan[group[j]];
            GridEncDesc d;
            std::memset(&d, 0, sizeof d);
            d.cells = d_cells[j] = (int32_t *)(c->d_enc_in.p + pl.cells_off);
            d.out = pl.direct ? c->d_cells.p + pl.off : c->d_enc_out.p + pl.scratch_off;
            d.lut = c->d_lut.p + pl.lut;
            d.lookup = (const int32_t *)(c->d_enc_in.p + pl.lookup_off);
            d.nx = g.nx; d.ny = g.ny; d.nz = g.nz; d.nbx = pl.rec.nbx; d.nby = pl.rec.nby; d.nbz = pl.rec.nbz;
            d.n_lookup = g.n_lookup;
            d.default_material = (g.default_material >= 0 && g.default_material < root->n_materials) ? g.default_material : -1;
            d.first_wg = first_wg[j];
            d.maskable = pl.rec.has_brick_mask ? 1u : 0u;
            descs[j] = d;
        }
        t0 = std::chrono::steady_clock::now();
        HIP_TRY(root, hipMemcpyAsync(c->d_enc_in.p, st, up_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(root, hipStreamSynchronize(c->stream));
        if (c == root) us[1] += us_since(t0);
        const int rc = src.on_device ? src.fill(root, c, group, c->d_enc_in.p + off_head, d_cells) : YCGE_OK;
        if (rc != YCGE_OK) return rc;
        t0 = std::chrono::steady_clock::now();
        const int e = ycge_launch_grid_encode(c->d_enc_in.p, (int)m, c->d_enc_in.p + off_res, n_wg, c->stream);
        if (e != 0) return root->fail(YCGE_ERR_DEVICE, "k_grid_encode launch failed: %s", hipGetErrorString((hipError_t)e));
        HIP_TRY(root, hipStreamSynchronize(c->stream));
        if (c == root) us[2] += us_since(t0);
        t0 = std::chrono::steady_clock::now();
        HIP_TRY(root, hipMemcpyAsync(st + off_back, c->d_enc_in.p + off_res, m * sizeof(GridEncResult), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(root, hipStreamSynchronize(c->stream));
        if (c == root) {
            us[3] += us_since(t0);
            for (size_t j = 0; j < m; j++) std::memcpy(&res[(size_t)group[j]], st + off_back + j * sizeof(GridEncResult), sizeof(GridEncResult));
        }
    }
    if (!src.caller_cells) {          // a pair with no material: named here, while the group's cells are still where they were made
        for (size_t j = 0; j < m; j++) {
            const size_t k = (size_t)group[j];
            const GridEncResult &r = res[k];
            if (r.bad_cell == 0xffffffffu) continue;
            int32_t pair[2] = {0, 0};
            if (!src.on_device) std::memcpy(pair, st + plan[k].cells_off + (size_t)r.bad_cell * 8, 8);
            else {
                HIP_TRY(root, hipSetDevice(root->device));
                const int rc = copy_out(root, pair, root->d_enc_in.p + plan[k].cells_off + (size_t)r.bad_cell * 8, 8);
                if (rc != YCGE_OK) return rc;
            }
            return root->fail(YCGE_ERR_INVALID_ARG, "%s: no material for (matId %d, metaId %d)", src.where(k, r.bad_cell).c_str(), pair[0], pair[1]);
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

// the body of ycge_scene_attach_grids, for any source of cells
int attach_grids_from(ycge_ctx *c, const ycge_grid *grids, int32_t n, int32_t *out_grid_index, CellSource &src)
{
    int rc = quiesce_all(c);
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
            P.recs.push_back(GGrid{}); P.codes.push_back(SlotCodes{}); P.resident.push_back(0); P.block_bytes.push_back(0); P.lut_region.push_back(-1);
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
    const std::vector<ycge_ctx *> ctxs = contexts_of(c);
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
    std::vector<int> group;
    size_t group_bytes = 0;
    const size_t budget = c->knobs.enc_group_bytes;          // (256 MiB; YCGE_ENC_GROUP_BYTES)
    for (int k = 0; k <= n; k++) {
        const size_t bytes = k < n ? (size_t)grids[k].nx * grids[k].ny * grids[k].nz * 8 : 0;
        if (!group.empty() && (k == n || group_bytes + bytes > budget)) {
            rc = encode_group(c, grids, plan, group, res, us, src);
            if (rc != YCGE_OK) return rc;
            group.clear(); group_bytes = 0;
        }
        if (k < n && plan[(size_t)k].device) { group.push_back(k); group_bytes += bytes; }
        if (group.size() >= src.group_max) group_bytes = budget;          // (a full group: the next grid opens a new one)
    }
    // ---- verdicts, records, the host encoder for the rest
    for (int k = 0; k < n; k++) {
        Planned &pl = plan[(size_t)k];
        const ycge_grid &g = grids[k];
        int lo[3], hi[3];
        uint64_t mask = 0;
        if (pl.device) {
            const GridEncResult &r = res[(size_t)k];
            if (r.bad_cell != 0xffffffffu)          // (cells that are not the caller's: encode_group has named it already)
                return c->fail(YCGE_ERR_INVALID_ARG, "grid %d: no material for (matId %d, metaId %d)", k, g.cells[2 * (size_t)r.bad_cell], g.cells[2 * (size_t)r.bad_cell + 1]);
            if (src.caller_cells && r.any_miss && too_many_pairs(g)) return c->fail(YCGE_ERR_UNSUPPORTED, "grid %d: more than 255 distinct (matId, metaId) pairs", k);
            if (src.foreign_cells && r.any_miss) {          // cells nobody has vetted (a world file's): the same limit, counted on a copy of the grid's cells
                std::vector<int32_t> made(2 * (size_t)g.nx * g.ny * g.nz);
                rc = src.write(c, (size_t)k, g, made.data());
                if (rc != YCGE_OK) return rc;
                ycge_grid gm = g;
                gm.cells = made.data();
                if (too_many_pairs(gm)) return c->fail(YCGE_ERR_UNSUPPORTED, "%s: more than 255 distinct (matId, metaId) pairs", src.where((size_t)k, CellSource::kNoCell).c_str());
            }
            for (int a = 0; a < 3; a++) { lo[a] = r.lo[a]; hi[a] = r.hi[a]; }
            mask = pl.rec.has_brick_mask ? ((uint64_t)r.mask_hi << 32) | r.mask_lo : 0;
            P.codes[(size_t)pl.index] = slot_codes_of(c, g, c->n_materials, nullptr, nullptr);
            P.device_encodes++;
        } else {
            pl.host_bytes.assign(pl.cap, 0);
            ycge_grid gh = g;
            std::vector<int32_t> made;
            if (!src.caller_cells) {
                made.resize(2 * (size_t)g.nx * g.ny * g.nz);
                rc = src.write(c, (size_t)k, g, made.data());
                if (rc != YCGE_OK) return rc;
                gh.cells = made.data();
            }
            std::vector<std::pair<int32_t, int32_t>> seen;
            rc = encode_grid_host(c, gh, k, c->n_materials, pl.rec, pl.host_bytes.data(), pl.host_lut, lo, hi, mask, &seen);
            if (rc != YCGE_OK) {          // (its refusals begin "grid k": cells that are not the caller's are named as their source names them)
                const std::string head = "grid " + std::to_string(k);
                if (!src.caller_cells && c->err.compare(0, head.size(), head) == 0) c->err = src.where((size_t)k, CellSource::kNoCell) + c->err.substr(head.size());
                return rc;
            }
            P.codes[(size_t)pl.index] = slot_codes_of(c, g, c->n_materials, &seen, pl.host_lut.data());
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
            // (the resident bytes AND this call's grids that still fitted the old arena: those were encoded in place, beyond d_cells.n)
            const size_t keep = x->d_cells.p ? std::max(x->d_cells.n, std::min<size_t>(x->d_cells.cap, (size_t)P.arena_end)) : 0;
            if (e == hipSuccess && keep) e = hipMemcpy(larger[i].p, x->d_cells.p, keep, hipMemcpyDeviceToDevice);
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

}  // namespace ycge_host

extern "C" {

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
    ycge_host::CallerCells src;
    return ycge_host::attach_grids_from(c, grids, n, out_grid_index, src);
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
        P.codes[i] = SlotCodes{};
        bounds[i] = std::array<float, 6>{{0, 0, 0, -1, -1, -1}};
        solid[i] = std::array<float, 7>{};
    }
    while (!P.recs.empty() && !P.resident.back()) {          // the tables follow the resident set: free slots at the end go
        P.free_index.erase((int32_t)P.recs.size() - 1);
        P.recs.pop_back(); P.codes.pop_back(); P.resident.pop_back(); P.block_bytes.pop_back(); P.lut_region.pop_back();
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
