// ycge_grid_edit.cpp - ycge_scene_edit_voxels: cells of resident grids changed where they lie (kernels: ycge_grid_edit.hip).
//
// THE PLAN is plain host code and decides every refusal before any device work: each op's grid must be resident and hold its box; its
// pair becomes a code byte by what the slot keeps (SlotCodes, ycge_ctx.h) - a device-encoded slot by its lookup table, a host-encoded
// slot by its first-seen pair list, which may grow up to code 255; the bricks the boxes touch become one work record each, and every
// record names the range of its grid's ops (grouped by grid, in list order).  A host-encoded grid of an upload holds its table packed
// between its neighbours': the first new code moves the table into a 256-entry region of the pool, as an attached grid has.
//
// COPY-THEN-COMMIT, as attach_grids_from does it: the plan works on copies of what it changes (the touched slots' code lists, the free
// LUT regions), the device work writes cells no refusal can follow, and the records, the pool and grid_solid take the new values in a
// last step that cannot fail.  (The LUT may have grown, contents kept, and new entries stand at codes no cell held: not observable.)
//
// THE RECORDS: k_grid_solid reduces the edited grids' solid boxes and brick masks, one small read-back brings them in, grid_record_solid
// makes the records.  When the record of a grid that an object holds changed, the objects are installed again from the kept list
// (update_objects, ycge_scene.cpp): the object record carries the box and the walk tree is derived from it.
#include <algorithm>

#include "ycge_ctx.h"
#include "ycge_grid_edit.h"

namespace ycge_host {

std::shared_ptr<const LookupTable> intern_lookup(ycge_ctx *root, const ycge_voxel_lookup *lookup, int32_t n)
{
    const size_t bytes = n > 0 ? (size_t)n * sizeof(ycge_voxel_lookup) : 0;
    std::string key(bytes ? (const char *)lookup : "", bytes);
    auto &tables = root->lookup_tables;
    auto it = tables.find(key);
    if (it != tables.end())
        if (auto held = it->second.lock()) return held;
    if (tables.size() >= 64)          // (tables nobody holds any more)
        for (auto i = tables.begin(); i != tables.end();) i = i->second.expired() ? tables.erase(i) : std::next(i);
    auto t = std::make_shared<LookupTable>();
    if (n > 0) t->e.assign(lookup, lookup + n);
    tables[std::move(key)] = t;
    return t;
}

SlotCodes slot_codes_of(ycge_ctx *root, const ycge_grid &g, int n_materials, const std::vector<std::pair<int32_t, int32_t>> *seen, const int32_t *lut)
{
    SlotCodes s;
    s.lookup = intern_lookup(root, g.lookup, g.n_lookup);
    s.default_material = (g.default_material >= 0 && g.default_material < n_materials) ? g.default_material : -1;
    if (seen) { s.host_encoded = true; s.seen = *seen; s.lut.assign(lut, lut + seen->size() + 1); }
    return s;
}

namespace {

const char *const kFn = "ycge_scene_edit_voxels";

struct Touched {
    int32_t gi = -1;
    SlotCodes codes;                    // a host-encoded slot: its copy, which the plan may extend
    bool new_codes = false;
    int32_t lut_region = -1;            // ... and then the region its table lies in afterwards (taken by this call when the slot had none)
    std::vector<GridEditOp> ops;
    std::vector<uint32_t> bricks;       // touched, sorted, once each
    GGrid rec;                          // the record afterwards
};

// the code byte of (mat, meta) in a slot; > 255: a refusal, its text in c->err
int resolve(ycge_ctx *c, int op, int32_t gi, const SlotCodes &fixed, SlotCodes *growing, int32_t mat, int32_t meta, uint32_t &code)
{
    if (mat <= 0) { code = 0; return YCGE_OK; }
    static const std::vector<ycge_voxel_lookup> no_table;
    const std::vector<ycge_voxel_lookup> &lk = fixed.lookup ? fixed.lookup->e : no_table;
    int hit = -1;
    if (!growing) {
        for (size_t k = 0; k < lk.size(); k++) if (lk[k].mat_id == mat && lk[k].meta_id == meta) { hit = (int)k; break; }
        if (hit >= 0) { code = (uint32_t)hit + 1; return YCGE_OK; }
        if (fixed.default_material >= 0) { code = (uint32_t)lk.size() + 1; return YCGE_OK; }
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: no material for (matId %d, metaId %d) in grid %d", kFn, op, mat, meta, gi);
    }
    for (size_t k = 0; k < growing->seen.size(); k++) if (growing->seen[k].first == mat && growing->seen[k].second == meta) { code = (uint32_t)k + 1; return YCGE_OK; }
    int material = growing->default_material;
    for (size_t k = 0; k < lk.size(); k++) if (lk[k].mat_id == mat && lk[k].meta_id == meta) { material = lk[k].material; break; }
    if (material < 0 || material >= c->n_materials) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: no material for (matId %d, metaId %d) in grid %d", kFn, op, mat, meta, gi);
    if (growing->seen.size() >= 255)
        return c->fail(YCGE_ERR_UNSUPPORTED, "%s: op %d: (matId %d, metaId %d) would be the 256th cell code of grid %d; codes of pairs no cell holds any more are not reclaimed: "
                       "detach the grid and attach it again", kFn, op, mat, meta, gi);
    growing->seen.push_back({mat, meta});
    growing->lut.push_back(material);
    code = (uint32_t)growing->seen.size();
    return YCGE_OK;
}

}  // namespace

int scene_edit_voxels(ycge_ctx *c, const ycge_voxel_edit *ops, int32_t n, uint32_t *out_info)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0 || n > YCGE_VOXEL_EDIT_MAX_OPS || (n > 0 && !ops)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad op array (n = %d; at most %d ops)", kFn, n, YCGE_VOXEL_EDIT_MAX_OPS);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) { if (out_info) std::memset(out_info, 0, 4 * sizeof(uint32_t)); return YCGE_OK; }

    // ---- the plan: every refusal is decided here
    const GridPool &P = c->grid_pool;
    std::vector<Touched> T;
    std::map<int32_t, size_t> touched_of;
    uint64_t n_bricks_listed = 0;
    for (int k = 0; k < n; k++) {
        const ycge_voxel_edit &e = ops[k];
        const int32_t gi = e.grid_index;
        if (gi < 0 || (size_t)gi >= P.recs.size() || !P.resident[(size_t)gi]) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: grid %d is not resident", kFn, k, gi);
        const GGrid &G = P.recs[(size_t)gi];
        const int dims[3] = {G.nx, G.ny, G.nz};
        for (int a = 0; a < 3; a++) {
            if (e.lo[a] > e.hi[a]) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: lo %d > hi %d on axis %d", kFn, k, e.lo[a], e.hi[a], a);
            if (e.lo[a] < 0 || e.hi[a] >= dims[a]) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: the box leaves grid %d (%d x %d x %d) on axis %d", kFn, k, gi, G.nx, G.ny, G.nz, a);
        }
        auto at = touched_of.find(gi);
        if (at == touched_of.end()) {
            at = touched_of.insert({gi, T.size()}).first;
            T.emplace_back();
            T.back().gi = gi; T.back().rec = G; T.back().lut_region = P.lut_region[(size_t)gi];
            if (P.codes[(size_t)gi].host_encoded) T.back().codes = P.codes[(size_t)gi];
        }
        Touched &t = T[at->second];
        const SlotCodes &fixed = P.codes[(size_t)gi];
        const size_t codes_before = t.codes.seen.size();
        GridEditOp op{};
        const int rc = resolve(c, k, gi, fixed, fixed.host_encoded ? &t.codes : nullptr, e.mat_id, e.meta_id, op.code);
        if (rc != YCGE_OK) return rc;
        if (t.codes.seen.size() != codes_before) t.new_codes = true;
        uint64_t span = 1;
        for (int a = 0; a < 3; a++) { op.lo[a] = e.lo[a]; op.hi[a] = e.hi[a]; span *= (uint64_t)((e.hi[a] >> 3) - (e.lo[a] >> 3) + 1); }
        n_bricks_listed += span;
        if (n_bricks_listed > YCGE_EDIT_MAX_RECORDS) return c->fail(YCGE_ERR_UNSUPPORTED, "%s: op %d: the boxes touch more than 2^26 bricks in one call", kFn, k);
        for (int bz = e.lo[2] >> 3; bz <= e.hi[2] >> 3; bz++)
            for (int by = e.lo[1] >> 3; by <= e.hi[1] >> 3; by++)
                for (int bx = e.lo[0] >> 3; bx <= e.hi[0] >> 3; bx++) t.bricks.push_back((uint32_t)((bz * G.nby + by) * G.nbx + bx));
        t.ops.push_back(op);
    }
    // a table that receives its first new code while it lies packed in the upload's takes a region of the pool
    std::vector<uint32_t> free_luts = P.free_luts;
    uint64_t lut_end = P.lut_end;
    size_t n_ops = 0, n_records = 0;
    uint64_t solid_wgs = 0;
    for (Touched &t : T) {
        std::sort(t.bricks.begin(), t.bricks.end());
        t.bricks.erase(std::unique(t.bricks.begin(), t.bricks.end()), t.bricks.end());
        n_ops += t.ops.size(); n_records += t.bricks.size();
        solid_wgs += ((uint64_t)t.rec.nbx * t.rec.nby * t.rec.nbz + 1) / 2;
        if (t.new_codes && t.lut_region < 0) {
            if (!free_luts.empty()) { t.lut_region = (int32_t)free_luts.back(); free_luts.pop_back(); }
            else {
                if (lut_end + YCGE_ENC_LUT_ENTRIES >= ((uint64_t)1 << 31)) return c->fail(YCGE_ERR_UNSUPPORTED, "voxel material tables exceed 2^31 entries");
                t.lut_region = (int32_t)lut_end; lut_end += YCGE_ENC_LUT_ENTRIES;
            }
            t.rec.lut_offset = (uint32_t)t.lut_region;
        }
    }
    if (solid_wgs >= 0x7fffffffull) return c->fail(YCGE_ERR_UNSUPPORTED, "%s: more bricks in the edited grids than one launch takes", kFn);

    // ---- the batch in page-locked staging: counters, results, descriptors, ops, records; the read-back lands behind it
    const size_t m = T.size();
    const size_t off_res = 256, off_desc = align_up(off_res + m * sizeof(GridEncResult), 256), off_ops = align_up(off_desc + m * sizeof(GridSolidDesc), 256);
    const size_t off_rec = align_up(off_ops + n_ops * sizeof(GridEditOp), 256), total = align_up(off_rec + n_records * sizeof(GridEditRecord), 256);
    const size_t back_bytes = off_res + m * sizeof(GridEncResult);
    int rc = quiesce_all(c);          // (the frames in flight read the cells)
    if (rc != YCGE_OK) return rc;
    const DeviceGuard guard(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->enc_stage.reserve(total + back_bytes, hipHostMallocPortable));
    uint8_t *st = c->enc_stage.data();
    std::memset(st, 0, off_res);
    {
        GridEncResult *res = (GridEncResult *)(st + off_res);
        GridSolidDesc *desc = (GridSolidDesc *)(st + off_desc);
        GridEditOp *dops = (GridEditOp *)(st + off_ops);
        GridEditRecord *recs = (GridEditRecord *)(st + off_rec);
        uint32_t op_at = 0, wg_at = 0;
        size_t rec_at = 0;
        for (size_t j = 0; j < m; j++) {
            const Touched &t = T[j];
            const GGrid &G = t.rec;
            GridEncResult r;
            std::memset(&r, 0, sizeof r);
            r.lo[0] = G.nx; r.lo[1] = G.ny; r.lo[2] = G.nz; r.hi[0] = r.hi[1] = r.hi[2] = -1; r.bad_cell = 0xffffffffu;
            res[j] = r;
            GridSolidDesc d{};
            d.cells = G.cell_offset; d.nbx = G.nbx; d.nby = G.nby; d.n_bricks = G.nbx * G.nby * G.nbz; d.first_wg = wg_at; d.maskable = G.has_brick_mask ? 1u : 0u;
            desc[j] = d;
            wg_at += (uint32_t)(((uint64_t)d.n_bricks + 1) / 2);
            std::memcpy(dops + op_at, t.ops.data(), t.ops.size() * sizeof(GridEditOp));
            for (uint32_t b : t.bricks) {
                GridEditRecord q{};
                q.brick = (uint64_t)G.cell_offset + (uint64_t)b * 512;
                q.bx = (int32_t)(b % (uint32_t)G.nbx); q.by = (int32_t)(b / (uint32_t)G.nbx % (uint32_t)G.nby); q.bz = (int32_t)(b / ((uint32_t)G.nbx * (uint32_t)G.nby));
                q.op_first = op_at; q.op_count = (uint32_t)t.ops.size();
                recs[rec_at++] = q;
            }
            op_at += (uint32_t)t.ops.size();
        }
    }

    // ---- every device: room for the tables, the new tables, the batch, the two kernels; the root's results come back
    for (ycge_ctx *x : contexts_of(c)) {
        HIP_TRY(c, hipSetDevice(x->device));
        const size_t lut_have = x->d_lut.p ? x->d_lut.cap : 0;
        if (lut_end > lut_have) {
            const hipError_t e = grow_preserve(x->d_lut, std::max<size_t>((size_t)lut_end, 2 * lut_have), x->d_lut.p ? x->d_lut.n : 0);
            x->sd.grid_lut = x->d_lut.p;
            HIP_TRY(c, e);
        }
        for (const Touched &t : T) {
            if (!t.new_codes) continue;
            std::vector<int32_t> lut = t.codes.lut;
            lut.resize(YCGE_ENC_LUT_ENTRIES, -1);
            HIP_TRY(c, hipMemcpy(x->d_lut.p + t.lut_region, lut.data(), YCGE_ENC_LUT_ENTRIES * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        if (x->d_lut.n < (size_t)lut_end) x->d_lut.n = (size_t)lut_end;
        if (x->d_enc_in.cap < total) HIP_TRY(c, x->d_enc_in.alloc(total));
        uint8_t *d = x->d_enc_in.p;
        HIP_TRY(c, hipMemcpyAsync(d, st, total, hipMemcpyHostToDevice, x->stream));
        int e = ycge_launch_grid_edit(x->d_cells.p, d + off_rec, (uint32_t)n_records, d + off_ops, (uint32_t *)d, x->stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_grid_edit launch failed: %s", hipGetErrorString((hipError_t)e));
        e = ycge_launch_grid_solid(x->d_cells.p, d + off_desc, (int)m, d + off_res, (uint32_t)solid_wgs, x->stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_grid_solid launch failed: %s", hipGetErrorString((hipError_t)e));
        if (x == c) HIP_TRY(c, hipMemcpyAsync(st + total, d, back_bytes, hipMemcpyDeviceToHost, x->stream));
        HIP_TRY(c, hipStreamSynchronize(x->stream));
    }
    HIP_TRY(c, hipSetDevice(c->device));

    // ---- the records that follow from the cells
    uint32_t info[4] = {0, 0, 0, 0};
    std::memcpy(info, st + total, 2 * sizeof(uint32_t));
    bool held_changed = false;
    for (size_t j = 0; j < m; j++) {
        Touched &t = T[j];
        GridEncResult r;
        std::memcpy(&r, st + total + off_res + j * sizeof(GridEncResult), sizeof r);
        const GGrid &old = P.recs[(size_t)t.gi];
        grid_record_solid(t.rec, r.lo, r.hi, t.rec.has_brick_mask ? ((uint64_t)r.mask_hi << 32) | r.mask_lo : 0);
        if (std::memcmp(t.rec.solid_lo, old.solid_lo, sizeof old.solid_lo) != 0 || std::memcmp(t.rec.solid_hi, old.solid_hi, sizeof old.solid_hi) != 0 ||
            t.rec.brick_mask_lo != old.brick_mask_lo || t.rec.brick_mask_hi != old.brick_mask_hi) {
            info[2]++;
            if ((size_t)t.gi < P.owner.size() && P.owner[(size_t)t.gi] >= 0) held_changed = true;
        }
    }
    for (ycge_ctx *x : contexts_of(c)) {
        HIP_TRY(c, hipSetDevice(x->device));
        for (const Touched &t : T)
            if (std::memcmp(&t.rec, &P.recs[(size_t)t.gi], sizeof(GGrid)) != 0) HIP_TRY(c, hipMemcpy(x->d_grids.p + t.gi, &t.rec, sizeof(GGrid), hipMemcpyHostToDevice));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // ---- nothing below fails (but the install of the objects, which leaves what ycge_scene_update_objects leaves)
    GridPool &Q = c->grid_pool;
    for (Touched &t : T) {
        const size_t i = (size_t)t.gi;
        Q.recs[i] = t.rec;
        if (t.new_codes) { Q.codes[i] = std::move(t.codes); Q.lut_region[i] = t.lut_region; }
        for (int a = 0; a < 3; a++) { c->grid_solid[i][a] = t.rec.solid_lo[a]; c->grid_solid[i][3 + a] = t.rec.solid_hi[a]; }
    }
    Q.free_luts.swap(free_luts);
    Q.lut_end = lut_end;
    if (held_changed) {
        rc = update_objects(c, c->last_prims.data(), (int32_t)c->last_prims.size());
        if (rc != YCGE_OK) return rc;
        info[3] = 1;
    } else {
        rc = query_scene_changed(c);
        if (rc != YCGE_OK) return rc;
    }
    if (out_info) std::memcpy(out_info, info, sizeof info);
    return YCGE_OK;
}

}  // namespace ycge_host
