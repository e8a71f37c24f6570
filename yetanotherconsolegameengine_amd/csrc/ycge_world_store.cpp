// ycge_world_store.cpp - a VG01 world resident on the device, and its chunks attached by key: the bodies of ycge_world_file_info,
// ycge_world_store_load / _info / _release, ycge_scene_attach_world_chunks and their hooks (the exports are in ycge_host.cpp).
//
// The reference reads a world file into preloadedWorld once (WorldManager.ReloadFromExistingFile, WorldManager.cs:399-508) and from then on
// every chunk that enters the view is a slice of that array (AttachChunkFromPreloaded, :696-752).  Here the payload goes up once and stays:
// the "world store", one allocation per device in VG01 order (x, then y, then z fastest, {mat, meta}).  An attach by key slices the chunks
// out of it on the device (k_ws_slice, ycge_world_store.hip) into the area k_grid_encode reads - a third CellSource behind attach_grids_from
// (ycge_grid_encode.cpp), beside the caller's cells and the generators' - so no cell crosses the bus again.
//
// LOAD: in x-slabs (a run of whole x-planes is contiguous in VG01 order) of YCGE_WORLD_STORE_SLAB_BYTES through two page-locked staging
// buffers, each slab staged once for all devices; a caller's range that is page-locked already is copied from directly.  Copies and the
// occupancy kernel run on two streams of the load's own, so the copy of slab k + 1 overlaps k_ws_occupied on slab k, and no stream of a
// frame is touched: a load joins no frame in flight.  The occupancy words come back once, after the last slab: which keys of an attach
// take part is decided on the host with no read-back.  The new store replaces the old one in a last step that cannot fail.
//
// YCGE_WORLD_STORE_HOST at ycge_create: the store is a host copy of the payload, the slice is a host loop and the cells go up as an
// attach's cells do - the yardstick and the fallback.
//
// GENERATE (ycge_world_store_generate): the store's source is the generator.  The reference makes the world once (GenerateAndSaveWorld),
// keeps it (ReloadFromExistingFile) and streams it (LoadChunksAround); here the window's 2-D fields are made on every device by the
// kernels of ycge_scene_generate_world (wp_make_fields, ycge_worldgen_cells.h) on streams of the call's own, and either STAY - the FIELDS
// form: tens of bytes a column, a chunk is made by k_wp_fill when its key is attached (FieldCells, WindowCells with the store's fields)
// - or are turned into the ordinary cell store by k_wp_planes, slab by slab, and freed (the CELLS form).  ycge_world_store_read hands
// the payload back in x-planes, whatever the store is made of: the way to a VG01 file that never holds the world in one piece.
#include <algorithm>

#include "ycge_worldgen_cells.h"

namespace ycge_host {
namespace {

const char *const kNoStore = "no world store loaded (ycge_world_store_load)";

size_t chunk_of(const WsShape &W, int cx, int cy, int cz) { return ((size_t)cx * W.ncy + cy) * W.ncz + cz; }
void clipped(const WsShape &W, int cx, int cy, int cz, int s[3])
{
    s[0] = std::min(W.S, W.nx - cx * W.S); s[1] = std::min(W.S, W.ny - cy * W.S); s[2] = std::min(W.S, W.nz - cz * W.S);          // WorldManager.cs:698-700
}
size_t first_cell(const WsShape &W, int cx, int cy, int cz) { return (((size_t)cx * W.S) * W.ny + (size_t)cy * W.S) * W.nz + (size_t)cz * W.S; }

// chunk `key` of a host world in VG01 order into `out`, ycge_grid.cells order (AttachChunkFromPreloaded's loop, :704-714)
void slice_host(const WsShape &W, const int32_t *world, const std::array<int32_t, 3> &key, int32_t *out)
{
    int s[3];
    clipped(W, key[0], key[1], key[2], s);
    const int32_t *base = world + 2 * first_cell(W, key[0], key[1], key[2]);
    for (size_t lx = 0; lx < (size_t)s[0]; lx++)
        for (size_t ly = 0; ly < (size_t)s[1]; ly++)
            std::memcpy(out + 2 * (lx * s[1] + ly) * s[2], base + 2 * ((lx * W.ny + ly) * W.nz), (size_t)s[2] * 8);
}

// chunk `key` of the root's device store into host memory: one k_ws_slice into a buffer of its own, one copy.  Nothing of the context may be in flight (copy_out).
int slice_to_host(ycge_ctx *c, const WorldStore &st, const std::array<int32_t, 3> &key, int32_t *out)
{
    const WsShape &W = st.shape;
    int s[3];
    clipped(W, key[0], key[1], key[2], s);
    const size_t n_cells = (size_t)s[0] * s[1] * s[2];
    const DeviceGuard guard(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint8_t> d;
    HIP_TRY(c, d.alloc(256 + n_cells * 8));
    WsChunk r{};
    r.src = first_cell(W, key[0], key[1], key[2]); r.sx = s[0]; r.sy = s[1]; r.sz = s[2]; r.dst = (int32_t *)(d.p + 256);
    HIP_TRY(c, hipMemcpy(d.p, &r, sizeof r, hipMemcpyHostToDevice));
    const int e = ycge_launch_world_store_slice(st.d_cells.p, &W, (const WsChunk *)d.p, 1, n_cells, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ws_slice launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return copy_out(c, out, d.p + 256, n_cells * 8);
}

// how a refusal names chunk `key` of the store, and cell `cell` of it (CellSource::where)
std::string chunk_where(const WsShape &W, const std::array<int32_t, 3> &key, uint32_t cell)
{
    int s[3];
    clipped(W, key[0], key[1], key[2], s);
    char buf[160];
    int n = std::snprintf(buf, sizeof buf, "ycge_scene_attach_world_chunks: chunk (%d, %d, %d)", key[0], key[1], key[2]);
    if (cell != CellSource::kNoCell) std::snprintf(buf + n, sizeof buf - (size_t)n, ", cell (%u, %u, %u)", cell / (uint32_t)(s[1] * s[2]), cell / (uint32_t)s[2] % (uint32_t)s[1], cell % (uint32_t)s[2]);
    return buf;
}

// chunk `key` of the root's fields store into host memory: one k_wp_fill into a buffer of its own, one copy.  Nothing of the context may be in flight (copy_out).
int fields_chunk_to_host(ycge_ctx *c, const WorldStore &st, const std::array<int32_t, 3> &key, int32_t *out)
{
    const size_t S = (size_t)st.shape.S, bytes = S * S * S * 8;
    const DeviceGuard guard(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint8_t> d;
    HIP_TRY(c, d.alloc(512 + bytes));
    uint8_t head[512] = {0};          // the chunk's record; at 256 its `any` word, zeroed
    const WgChunk r{key[0], key[1], key[2], 0, (int32_t *)(d.p + 512)};
    std::memcpy(head, &r, sizeof r);
    HIP_TRY(c, hipMemcpy(d.p, head, sizeof head, hipMemcpyHostToDevice));
    WpFields F;
    wp_layout(st.d_fields.p, (size_t)st.gen_window.nx * st.gen_window.nz, 0, &F);
    const int e = ycge_launch_worldpregen_fill((const WgChunk *)d.p, 1, &st.gen_world, &st.gen_window, &F, (uint32_t *)(d.p + 256), c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_fill launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return copy_out(c, out, d.p + 512, bytes);
}

// ... and as every reader sees it: out of its slot of the edit pool when it holds one, made from the fields otherwise
int chunk_to_host(ycge_ctx *c, const WorldStore &st, const std::array<int32_t, 3> &key, int32_t *out)
{
    const int slot = st.pool_cap ? st.slot_of[chunk_of(st.shape, key[0], key[1], key[2])] : -1;
    if (slot < 0) return fields_chunk_to_host(c, st, key, out);
    const size_t S = (size_t)st.shape.S;
    const DeviceGuard guard(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return copy_out(c, out, st.d_pool.p + (size_t)slot * st.pool_stride, S * S * S * 8);
}

// the chunks of one ycge_scene_attach_world_chunks on a fields store: ycge_scene_generate_world's source, filling from the fields the store keeps
struct FieldCells : WindowCells {
    WorldStore &store;                     // the root's
    explicit FieldCells(WorldStore &s) : WindowCells("ycge_scene_attach_world_chunks", s.gen_world, true, s.gen_window), store(s) {}
    uint8_t *fields_of(ycge_ctx *x) const override { return x->world_store.d_fields.p; }
    std::string where(size_t k, uint32_t cell) const override { return chunk_where(store.shape, keys[k], cell); }
    // for the host encoder (a lookup table k_grid_encode does not take)
    int write(ycge_ctx *root, size_t k, const ycge_grid &, int32_t *cells) override { return chunk_to_host(root, store, keys[k], cells); }
    int slot_of(size_t k) const { return store.pool_cap ? store.slot_of[chunk_of(store.shape, keys[k][0], keys[k][1], keys[k][2])] : -1; }
    // the generator's records and `any` words for a group of m, then a copy record for every chunk of the group that holds a slot of the
    // pool.  fill_chunks sends GeneratedCells::head_bytes(m') bytes for the m' <= m chunks it makes, so it writes inside the generator's
    // part and never reaches the copy records, which a kernel in flight may still be reading.
    size_t head_bytes(size_t m) const override { return WindowCells::head_bytes(m) + align_up(m * sizeof(WsPoolCopy), 256); }
    // a chunk that holds a slot is copied out of it (k_ws_pool_copy, one launch for the group's); the others are made from the fields as ever
    int fill(ycge_ctx *root, ycge_ctx *x, const std::vector<int> &group, uint8_t *d_head, const std::vector<int32_t *> &d_cells) override
    {
        if (!store.pool_used) return WindowCells::fill(root, x, group, d_head, d_cells);
        std::vector<int> made;
        std::vector<int32_t *> made_cells;
        std::vector<WsPoolCopy> copies;
        for (size_t j = 0; j < group.size(); j++) {
            const int slot = slot_of((size_t)group[j]);
            if (slot < 0) { made.push_back(group[j]); made_cells.push_back(d_cells[j]); }
            else copies.push_back(WsPoolCopy{slot, 0, d_cells[j]});
        }
        if (!copies.empty()) {
            uint8_t *d_copies = d_head + WindowCells::head_bytes(group.size());
            HIP_TRY(root, hipMemcpy(d_copies, copies.data(), copies.size() * sizeof(WsPoolCopy), hipMemcpyHostToDevice));
            const WorldStore &xs = x->world_store;
            const int e = ycge_launch_world_store_pool_copy(xs.d_pool.p, store.pool_stride, store.shape.S, (const WsPoolCopy *)d_copies, (int)copies.size(), x->stream);
            if (e != 0) return root->fail(YCGE_ERR_DEVICE, "k_ws_pool_copy launch failed: %s", hipGetErrorString((hipError_t)e));
        }
        return made.empty() ? YCGE_OK : fill_chunks(root, x, made, d_head, made_cells);
    }
};

// the chunks of one ycge_scene_attach_world_chunks: grid k of the attach is chunk keys[k]
struct StoreCells : CellSource {
    WorldStore &store;                     // the root's
    std::vector<std::array<int32_t, 3>> keys;
    explicit StoreCells(WorldStore &s) : store(s) { on_device = !s.on_host; foreign_cells = true; group_max = 32768; }          // (gridDim.y of a slice launch)
    size_t head_bytes(size_t m) const override { return align_up(m * sizeof(WsChunk), 256); }
    std::string where(size_t k, uint32_t cell) const override { return chunk_where(store.shape, keys[k], cell); }
    // the host store's slice; or, for the host encoder (a lookup table k_grid_encode does not take) and the count of distinct pairs, the chunk sliced out of the device store
    int write(ycge_ctx *root, size_t k, const ycge_grid &, int32_t *cells) override
    {
        if (store.on_host) { slice_host(store.shape, store.host_cells.data(), keys[k], cells); return YCGE_OK; }
        return slice_to_host(root, store, keys[k], cells);
    }
    int fill(ycge_ctx *root, ycge_ctx *x, const std::vector<int> &group, uint8_t *d_head, const std::vector<int32_t *> &d_cells) override
    {
        const WsShape &W = store.shape;
        std::vector<WsChunk> recs(group.size());
        size_t max_cells = 0;
        for (size_t j = 0; j < group.size(); j++) {
            const auto &key = keys[(size_t)group[j]];
            WsChunk r{};
            r.src = first_cell(W, key[0], key[1], key[2]);
            int s[3];
            clipped(W, key[0], key[1], key[2], s);
            r.sx = s[0]; r.sy = s[1]; r.sz = s[2]; r.dst = d_cells[j];
            max_cells = std::max(max_cells, (size_t)s[0] * s[1] * s[2]);
            recs[j] = r;
        }
        HIP_TRY(root, hipMemcpy(d_head, recs.data(), recs.size() * sizeof(WsChunk), hipMemcpyHostToDevice));
        // the encode launch follows on the same stream: nothing waits here.  The root's launch lies between two events the stats hook reads later.
        Event *ev = nullptr;
        if (x == root) {
            if (store.slice_ev.size() < store.slice_ev_used + 2) store.slice_ev.resize(store.slice_ev_used + 2);
            ev = &store.slice_ev[store.slice_ev_used];
            HIP_TRY(root, ev[0].ensure(hipEventDefault)); HIP_TRY(root, ev[1].ensure(hipEventDefault));
            HIP_TRY(root, hipEventRecord(ev[0], x->stream));
        }
        const int e = ycge_launch_world_store_slice(x->world_store.d_cells.p, &W, (const WsChunk *)d_head, (int)recs.size(), max_cells, x->stream);
        if (e != 0) return root->fail(YCGE_ERR_DEVICE, "k_ws_slice launch failed: %s", hipGetErrorString((hipError_t)e));
        if (ev) { HIP_TRY(root, hipEventRecord(ev[1], x->stream)); store.slice_ev_used += 2; }
        return YCGE_OK;
    }
};

int need_root(ycge_ctx *c)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    return YCGE_OK;
}

}  // namespace

int world_file_info(const uint8_t *bytes, size_t n_bytes, int32_t dims_out[3], size_t *payload_offset_out, char *msg, size_t msg_bytes)
{
    auto refuse = [&](const char *why) { if (msg && msg_bytes) std::snprintf(msg, msg_bytes, "%s", why); return (int)YCGE_ERR_INVALID_ARG; };
    if (msg && msg_bytes) msg[0] = 0;
    if (!bytes || !dims_out) return refuse("ycge_world_file_info: null argument");
    const char *const eof = "Unable to read beyond the end of the stream.";
    // ReloadFromExistingFile, :414-424: four ReadChar, THEN the compare, then three ReadInt32 - a read that runs out of bytes throws
    if (n_bytes < 4) return refuse(eof);
    if (std::memcmp(bytes, "VG01", 4) != 0) return refuse("Unsupported world file header. Expected 'VG01'.");
    if (n_bytes < 16) return refuse(eof);
    int32_t d[3];
    for (int a = 0; a < 3; a++) {
        const uint8_t *p = bytes + 4 + 4 * a;
        d[a] = (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    }
    if (d[0] <= 0 || d[1] <= 0 || d[2] <= 0) return refuse("Invalid world dimensions.");
    const uint64_t cells = (uint64_t)d[0] * (uint64_t)d[1] * (uint64_t)d[2];          // (< 2^93 in exact arithmetic: compare before it can wrap)
    if ((uint64_t)d[0] * (uint64_t)d[1] >= ((uint64_t)1 << 30) || cells >= ((uint64_t)1 << 30)) return refuse("ycge_world_file_info: nx * ny * nz >= 2^30");
    if (n_bytes - 16 < 8 * cells) return refuse(eof);
    for (int a = 0; a < 3; a++) dims_out[a] = d[a];
    if (payload_offset_out) *payload_offset_out = 16;
    return YCGE_OK;
}

int world_store_load(ycge_ctx *c, const int32_t *cells, int32_t nx, int32_t ny, int32_t nz, int32_t chunk_size)
{
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    if (!cells) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_load: null cells");
    if (nx <= 0 || ny <= 0 || nz <= 0) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_load: dimensions %d x %d x %d", nx, ny, nz);
    if ((uint64_t)nx * (uint64_t)ny >= ((uint64_t)1 << 30) || (uint64_t)nx * (uint64_t)ny * (uint64_t)nz >= ((uint64_t)1 << 30))
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_load: nx * ny * nz >= 2^30");
    if (chunk_size < 1 || chunk_size > YCGE_WORLD_STORE_MAX_CHUNK) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_load: chunk_size %d is outside 1..%d", chunk_size, YCGE_WORLD_STORE_MAX_CHUNK);
    WsShape W{};
    W.nx = nx; W.ny = ny; W.nz = nz; W.S = chunk_size;
    W.ncx = (nx + chunk_size - 1) / chunk_size; W.ncy = (ny + chunk_size - 1) / chunk_size; W.ncz = (nz + chunk_size - 1) / chunk_size;
    const uint64_t n_chunks64 = (uint64_t)W.ncx * (uint64_t)W.ncy * (uint64_t)W.ncz;
    if (n_chunks64 > (uint64_t)YCGE_WORLD_STORE_MAX_CHUNKS) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_load: more than 2^24 chunks");
    const size_t n_chunks = (size_t)n_chunks64, plane_cells = (size_t)ny * nz, n_i32 = 2 * (size_t)nx * plane_cells, total = n_i32 * 4;

    const std::vector<ycge_ctx *> ctxs = contexts_of(c);
    std::vector<WorldStore> made(ctxs.size());          // every device's new store, complete before any context takes its own
    WorldStore &R = made[0];
    for (WorldStore &s : made) { s.held = true; s.shape = W; }
    R.occupied.assign(n_chunks, 0);
    R.bytes = (int64_t)total;
    if (c->knobs.world_store_host) {
        R.on_host = true;
        const auto t0 = std::chrono::steady_clock::now();
        R.host_cells.assign(cells, cells + n_i32);
        for (size_t x = 0; x < (size_t)nx; x++)
            for (size_t y = 0; y < (size_t)ny; y++) {
                const int32_t *row = cells + 2 * ((x * ny + y) * nz);
                uint8_t *occ = R.occupied.data() + chunk_of(W, (int)(x / chunk_size), (int)(y / chunk_size), 0);
                for (size_t z = 0; z < (size_t)nz; z++)
                    if (row[2 * z] != 0) occ[z / chunk_size] = 1;          // Item1 != 0, :716
            }
        R.load_us[0] = us_since(t0);
        for (size_t i = 1; i < made.size(); i++) made[i].on_host = true;
    } else {
        const DeviceGuard guard(c->device);
        const size_t plane_bytes = plane_cells * 8;
        const size_t planes = std::max<size_t>(1, std::min<size_t>((size_t)nx, c->knobs.world_store_slab_bytes / plane_bytes));          // per slab
        const bool direct = host_memory_is_page_locked(cells, total);
        PinnedBuf stage[2], occ_back;
        Stream copy_s[YCGE_MAX_DEVICES], kern_s;
        Event copied[YCGE_MAX_DEVICES][2], c_begin[2], k_begin[2], k_end[2];
        DevBuf<uint32_t> d_occ;
        if (ctxs.size() > YCGE_MAX_DEVICES) return c->fail(YCGE_ERR_INTERNAL, "ycge_world_store_load: %d devices", (int)ctxs.size());
        for (size_t i = 0; i < ctxs.size(); i++) {
            HIP_TRY(c, hipSetDevice(ctxs[i]->device));
            HIP_TRY(c, made[i].d_cells.alloc(n_i32));
            HIP_TRY(c, copy_s[i].ensure());
            for (int b = 0; b < 2; b++) HIP_TRY(c, copied[i][b].ensure(hipEventDefault));
        }
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, kern_s.ensure());
        for (int b = 0; b < 2; b++) { HIP_TRY(c, c_begin[b].ensure(hipEventDefault)); HIP_TRY(c, k_begin[b].ensure(hipEventDefault)); HIP_TRY(c, k_end[b].ensure(hipEventDefault)); }
        HIP_TRY(c, d_occ.alloc(n_chunks));
        HIP_TRY(c, hipMemsetAsync(d_occ.p, 0, n_chunks * 4, kern_s));
        HIP_TRY(c, occ_back.reserve(n_chunks * 4));
        if (!direct) for (int b = 0; b < (planes < (size_t)nx ? 2 : 1); b++) HIP_TRY(c, stage[b].reserve(planes * plane_bytes, hipHostMallocPortable));          // (every device copies from it; one slab: one buffer)
        // slab k - 2, which went through buffer b, is done with: its copies on every device, its kernel; the root's times taken
        auto collect = [&](int b) -> int {
            for (size_t i = 1; i < ctxs.size(); i++) HIP_TRY(c, hipEventSynchronize(copied[i][b]));
            HIP_TRY(c, hipEventSynchronize(k_end[b]));
            float ms = 0;
            HIP_TRY(c, hipEventElapsedTime(&ms, c_begin[b], copied[0][b])); R.load_us[1] += 1000.0 * ms;
            HIP_TRY(c, hipEventElapsedTime(&ms, k_begin[b], k_end[b])); R.load_us[2] += 1000.0 * ms;
            return YCGE_OK;
        };
        size_t k = 0;
        for (size_t x0 = 0; x0 < (size_t)nx; x0 += planes, k++) {
            const int b = (int)(k & 1);
            const size_t px = std::min(planes, (size_t)nx - x0), off_i32 = 2 * x0 * plane_cells, bytes = px * plane_bytes;
            if (k >= 2) { rc = collect(b); if (rc != YCGE_OK) return rc; }
            const int32_t *from = cells + off_i32;
            if (!direct) {
                const auto t0 = std::chrono::steady_clock::now();
                std::memcpy(stage[b].p, from, bytes);
                R.load_us[0] += us_since(t0);
                from = (const int32_t *)stage[b].p;
            }
            for (size_t i = 0; i < ctxs.size(); i++) {
                HIP_TRY(c, hipSetDevice(ctxs[i]->device));
                if (i == 0) HIP_TRY(c, hipEventRecord(c_begin[b], copy_s[0]));
                HIP_TRY(c, hipMemcpyAsync(made[i].d_cells.p + off_i32, from, bytes, hipMemcpyHostToDevice, copy_s[i]));
                HIP_TRY(c, hipEventRecord(copied[i][b], copy_s[i]));
            }
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, hipStreamWaitEvent(kern_s, copied[0][b], 0));
            HIP_TRY(c, hipEventRecord(k_begin[b], kern_s));
            const int e = ycge_launch_world_store_occupied(R.d_cells.p, &W, (int32_t)x0, (int32_t)px, d_occ.p, kern_s);
            if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ws_occupied launch failed: %s", hipGetErrorString((hipError_t)e));
            HIP_TRY(c, hipEventRecord(k_end[b], kern_s));
        }
        R.slabs = (int64_t)k;
        for (size_t j = (k >= 2 ? k - 2 : 0); j < k; j++) { rc = collect((int)(j & 1)); if (rc != YCGE_OK) return rc; }
        HIP_TRY(c, hipMemcpyAsync(occ_back.p, d_occ.p, n_chunks * 4, hipMemcpyDeviceToHost, kern_s));
        HIP_TRY(c, hipStreamSynchronize(kern_s));
        for (size_t i = 0; i < ctxs.size(); i++) { HIP_TRY(c, hipSetDevice(ctxs[i]->device)); HIP_TRY(c, hipStreamSynchronize(copy_s[i])); }
        const uint32_t *words = (const uint32_t *)occ_back.p;
        for (size_t i = 0; i < n_chunks; i++) R.occupied[i] = words[i] != 0;
    }
    // ---- nothing below fails: the new store replaces the old one (whose memory goes with it); the counters go on
    R.device_chunks = c->world_store.device_chunks; R.host_chunks = c->world_store.host_chunks;
    for (size_t i = 0; i < ctxs.size(); i++) {
        (void)hipSetDevice(ctxs[i]->device);
        ctxs[i]->world_store = std::move(made[i]);
    }
    (void)hipSetDevice(c->device);
    return YCGE_OK;
}

int world_store_info(ycge_ctx *c, int32_t dims_out[3], int32_t *chunk_size_out, uint8_t *occupied_out, size_t capacity)
{
    const int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    const WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    if (occupied_out && capacity < st.occupied.size()) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_info: %zu chunks, room for %zu", st.occupied.size(), capacity);
    if (dims_out) { dims_out[0] = st.shape.nx; dims_out[1] = st.shape.ny; dims_out[2] = st.shape.nz; }
    if (chunk_size_out) *chunk_size_out = st.shape.S;
    if (occupied_out) std::memcpy(occupied_out, st.occupied.data(), st.occupied.size());
    return YCGE_OK;
}

int world_store_release(ycge_ctx *c)
{
    const int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    const int64_t dev = c->world_store.device_chunks, host = c->world_store.host_chunks;
    for (ycge_ctx *x : contexts_of(c)) { (void)hipSetDevice(x->device); x->world_store = WorldStore{}; }
    (void)hipSetDevice(c->device);
    c->world_store.device_chunks = dev; c->world_store.host_chunks = host;
    return YCGE_OK;
}

int world_store_attach(ycge_ctx *c, const int32_t *keys, int32_t n, const ycge_grid *proto, int32_t *out_grid_index)
{
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    if (n < 0 || (n > 0 && (!keys || !out_grid_index)) || !proto) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_attach_world_chunks: bad array (n = %d)", n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    if (n == 0) return YCGE_OK;
    const WsShape &W = st.shape;
    static const int32_t no_cells[2] = {0, 0};          // (validate_grid wants a pointer; these grids' cells are never read through it)
    ycge_grid g0 = *proto;
    g0.nx = std::min(W.S, W.nx); g0.ny = std::min(W.S, W.ny); g0.nz = std::min(W.S, W.nz); g0.cells = no_cells;          // (the largest chunk)
    std::string m;
    const int vrc = validate_grid(g0, 0, c->n_materials, m);
    if (vrc != YCGE_OK) return c->fail(vrc, "%s", m.c_str());
    // which keys take a grid: inside the chunk counts (the reference's index exception otherwise, swallowed in EnsureViewLoaded) and occupied (:716-718)
    StoreCells store_src(st);
    FieldCells field_src(st);          // (a fields store: the generator's source, filling from the resident fields)
    CellSource &src = st.fields ? (CellSource &)field_src : (CellSource &)store_src;
    std::vector<std::array<int32_t, 3>> &src_keys = st.fields ? field_src.keys : store_src.keys;
    std::vector<ycge_grid> grids;
    std::vector<int> which;
    for (int k = 0; k < n; k++) {
        const int32_t cx = keys[3 * k], cy = keys[3 * k + 1], cz = keys[3 * k + 2];
        if (cx < 0 || cy < 0 || cz < 0 || cx >= W.ncx || cy >= W.ncy || cz >= W.ncz || !st.occupied[chunk_of(W, cx, cy, cz)]) continue;
        int s[3];
        clipped(W, cx, cy, cz, s);
        ycge_grid g = g0;
        g.nx = s[0]; g.ny = s[1]; g.nz = s[2];
        g.min_corner.x = proto->min_corner.x + (float)(cx * W.S) * proto->voxel_size.x;          // :720-724, as chunk_grid (ycge_worldgen_scene.cpp)
        g.min_corner.y = proto->min_corner.y + (float)(cy * W.S) * proto->voxel_size.y;
        g.min_corner.z = proto->min_corner.z + (float)(cz * W.S) * proto->voxel_size.z;
        grids.push_back(g); which.push_back(k); src_keys.push_back({{cx, cy, cz}});
    }
    std::vector<int32_t> idx(grids.size(), -1);
    field_src.col.assign(src_keys.size(), 0);
    st.slice_ev_used = 0; st.last_fill_us = 0;
    rc = grids.empty() ? YCGE_OK : attach_grids_from(c, grids.data(), (int32_t)grids.size(), idx.data(), src);
    st.last_fill_us = field_src.fill_us;
    if (rc != YCGE_OK) return rc;
    std::fill(out_grid_index, out_grid_index + n, -1);
    for (size_t j = 0; j < which.size(); j++) out_grid_index[which[j]] = idx[j];
    // who sliced: the kernel, or the host (the knob; the device store's rows for the host encoder, a lookup table k_grid_encode does not take)
    (src.on_device && proto->n_lookup <= YCGE_ENC_MAX_LOOKUP ? st.device_chunks : st.host_chunks) += (int64_t)grids.size();
    return YCGE_OK;
}

int world_store_chunk(ycge_ctx *c, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t dims_out[3])
{
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    const WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    const WsShape &W = st.shape;
    if (cx < 0 || cy < 0 || cz < 0 || cx >= W.ncx || cy >= W.ncy || cz >= W.ncz) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_debug_world_store_chunk: no chunk (%d, %d, %d)", cx, cy, cz);
    int s[3];
    clipped(W, cx, cy, cz, s);
    if (dims_out) for (int a = 0; a < 3; a++) dims_out[a] = s[a];
    if (!cells_out) return YCGE_OK;
    if (st.on_host) { slice_host(W, st.host_cells.data(), {{cx, cy, cz}}, cells_out); return YCGE_OK; }
    rc = quiesce(c);          // (copy_out's staging is the frames' too)
    if (rc != YCGE_OK) return rc;
    if (st.fields) return chunk_to_host(c, st, {{cx, cy, cz}}, cells_out);
    return slice_to_host(c, st, {{cx, cy, cz}}, cells_out);
}

int world_store_stats(ycge_ctx *c, int64_t *out8)
{
    if (!c || !out8) return YCGE_ERR_INVALID_ARG;
    const WorldStore &st = c->world_store;
    out8[0] = st.held ? st.bytes : 0; out8[1] = st.slabs;
    for (int a = 0; a < 3; a++) out8[2 + a] = (int64_t)st.load_us[a];
    double slice_us = 0;          // the last attach's slice launches, a pair of events per group (the attach has ended: they are all recorded and complete)
    for (size_t i = 0; i + 1 < st.slice_ev_used; i += 2) {
        float ms = 0;
        HIP_TRY(c, hipEventSynchronize(st.slice_ev[i + 1]));
        HIP_TRY(c, hipEventElapsedTime(&ms, st.slice_ev[i], st.slice_ev[i + 1]));
        slice_us += 1000.0 * ms;
    }
    if (st.held && st.fields) slice_us = st.last_fill_us;          // (a fields store slices nothing: its chunks are made by k_wp_fill)
    out8[5] = (int64_t)slice_us; out8[6] = st.device_chunks; out8[7] = st.host_chunks;
    return YCGE_OK;
}

int world_store_generate(ycge_ctx *c, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t form)
{
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    const char *why = nullptr;
    if (worldgen_check(world, &why) != YCGE_OK || worldgen_window_check(world, chunks_x, chunks_z, origin_bx, origin_bz, &why) != YCGE_OK)
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_generate: %s", why);
    if (form != YCGE_WORLD_STORE_FIELDS && form != YCGE_WORLD_STORE_CELLS) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_generate: form %d", form);
    const int S = world->chunk_size, chunks_y = world->chunks_y;
    const wg::World gW = wg::make_world(S, chunks_y, world->world_seed);
    const wg::Window gN{chunks_x * S, chunks_z * S, origin_bx, origin_bz};
    WsShape W{};
    W.nx = gN.nx; W.ny = gW.height; W.nz = gN.nz; W.S = S; W.ncx = chunks_x; W.ncy = chunks_y; W.ncz = chunks_z;
    const size_t n_cols = (size_t)W.nx * W.nz, n_chunks = (size_t)chunks_x * chunks_y * chunks_z, plane_cells = (size_t)W.ny * W.nz, n_i32 = 2 * n_cols * (size_t)W.ny;
    if (n_chunks > (size_t)YCGE_WORLD_STORE_MAX_CHUNKS) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_generate: more than 2^24 chunks");

    if (c->knobs.worldgen_host || c->knobs.world_store_host) {          // the host generator's cells, loaded as any payload is: the fallback and a second yardstick
        std::vector<int32_t> cells(n_i32);
        const auto t0 = std::chrono::steady_clock::now();
        world_cells_host(world, chunks_x, chunks_z, origin_bx, origin_bz, cells.data());
        const double host_us = us_since(t0);
        rc = world_store_load(c, cells.data(), W.nx, W.ny, W.nz, S);
        if (rc != YCGE_OK) return rc;
        WorldStore &st = c->world_store;
        st.gen_form = form; st.gen_on_host = 1; st.gen_passes = 0; st.gen_slabs = st.slabs;
        for (double &u : st.gen_us) u = 0;
        st.gen_us[4] = host_us;
        return YCGE_OK;
    }

    const DeviceGuard guard(c->device);
    const std::vector<ycge_ctx *> ctxs = contexts_of(c);
    if (ctxs.size() > YCGE_MAX_DEVICES) return c->fail(YCGE_ERR_INTERNAL, "ycge_world_store_generate: %d devices", (int)ctxs.size());
    std::vector<WorldStore> made(ctxs.size());          // every device's new store, complete before any context takes its own
    WorldStore &R = made[0];
    for (WorldStore &s : made) { s.held = true; s.shape = W; s.gen_world = gW; s.gen_window = gN; }
    const size_t fields_bytes = wp_layout(nullptr, n_cols, n_chunks, nullptr);
    Stream gen_s[YCGE_MAX_DEVICES];          // the call's own: no stream of a frame is touched
    PinnedBuf back;                          // the flip counts and the occupancy words come back through it
    HIP_TRY(c, back.reserve(std::max<size_t>(256, n_chunks * 4)));
    std::vector<uint32_t> words(n_chunks, 0);
    int passes = 0;
    for (size_t i = 0; i < ctxs.size(); i++) {          // (the root first: a peer repeats its passes without reading anything back)
        HIP_TRY(c, hipSetDevice(ctxs[i]->device));
        HIP_TRY(c, made[i].d_fields.alloc(fields_bytes));
        HIP_TRY(c, gen_s[i].ensure());
        const hipStream_t s = gen_s[i];
        const WpReadBack read_back = [&](void *dst, const void *from, size_t bytes) -> int {
            HIP_TRY(c, hipMemcpyAsync(back.p, from, bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(c, hipStreamSynchronize(s));
            std::memcpy(dst, back.p, bytes);
            return YCGE_OK;
        };
        rc = wp_make_fields(c, "ycge_world_store_generate", i == 0, made[i].d_fields.p, gW, gN, chunks_y, chunks_z, s, read_back, passes, R.gen_us, words.data());
        if (rc != YCGE_OK) return rc;
    }
    R.occupied.assign(n_chunks, 0);
    for (size_t k = 0; k < n_chunks; k++) R.occupied[k] = words[k] != 0;
    R.gen_form = form; R.gen_passes = passes;
    if (form == YCGE_WORLD_STORE_FIELDS) {
        for (WorldStore &s : made) s.fields = true;
        R.bytes = (int64_t)fields_bytes;
        R.gen_occupied = R.occupied;          // (what ycge_world_store_revert_chunks gives a chunk back)
    } else {
        // the cell store, written where it will lie: x-slabs of k_wp_planes on every device, and on the root k_ws_occupied behind each slab -
        // the loaded store's occupancy kernel on the generated cells, which must find what k_wp_occupied found in the fields
        const size_t plane_bytes = plane_cells * 8;
        const size_t planes = std::max<size_t>(1, std::min<size_t>((size_t)W.nx, c->knobs.world_store_slab_bytes / plane_bytes));          // per slab
        DevBuf<uint32_t> d_occ;
        Event k_begin, k_end;
        size_t slabs = 0;
        for (size_t i = 0; i < ctxs.size(); i++) {
            HIP_TRY(c, hipSetDevice(ctxs[i]->device));
            HIP_TRY(c, made[i].d_cells.alloc(n_i32));
            WpFields F;
            wp_layout(made[i].d_fields.p, n_cols, n_chunks, &F);
            if (i == 0) {
                HIP_TRY(c, d_occ.alloc(n_chunks));
                HIP_TRY(c, hipMemsetAsync(d_occ.p, 0, n_chunks * 4, gen_s[0]));
                HIP_TRY(c, k_begin.ensure(hipEventDefault)); HIP_TRY(c, k_end.ensure(hipEventDefault));
                HIP_TRY(c, hipEventRecord(k_begin, gen_s[0]));
            }
            for (size_t x0 = 0; x0 < (size_t)W.nx; x0 += planes) {
                const size_t px = std::min(planes, (size_t)W.nx - x0);
                int e = ycge_launch_worldpregen_planes(&gW, &gN, &F, (int32_t)x0, (int32_t)px, made[i].d_cells.p + 2 * x0 * plane_cells, gen_s[i]);
                if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_planes launch failed: %s", hipGetErrorString((hipError_t)e));
                if (i != 0) continue;
                slabs++;
                e = ycge_launch_world_store_occupied(R.d_cells.p, &W, (int32_t)x0, (int32_t)px, d_occ.p, gen_s[0]);
                if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ws_occupied launch failed: %s", hipGetErrorString((hipError_t)e));
            }
            if (i == 0) HIP_TRY(c, hipEventRecord(k_end, gen_s[0]));
        }
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipMemcpyAsync(back.p, d_occ.p, n_chunks * 4, hipMemcpyDeviceToHost, gen_s[0]));
        for (size_t i = 0; i < ctxs.size(); i++) { HIP_TRY(c, hipSetDevice(ctxs[i]->device)); HIP_TRY(c, hipStreamSynchronize(gen_s[i])); }
        HIP_TRY(c, hipSetDevice(c->device));
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, k_begin, k_end));
        R.gen_us[3] = 1000.0 * ms;
        const uint32_t *seen = (const uint32_t *)back.p;
        for (size_t k = 0; k < n_chunks; k++)
            if ((seen[k] != 0) != (R.occupied[k] != 0))
                return c->fail(YCGE_ERR_INTERNAL, "ycge_world_store_generate: k_wp_occupied and k_ws_occupied disagree on chunk (%d, %d, %d)", (int)(k / ((size_t)chunks_y * chunks_z)),
                               (int)(k / (size_t)chunks_z % (size_t)chunks_y), (int)(k % (size_t)chunks_z));
        for (WorldStore &s : made) s.d_fields.release();          // (the cells are the store: the fields have done their work)
        R.bytes = (int64_t)(n_i32 * 4); R.slabs = R.gen_slabs = (int64_t)slabs;
    }
    // ---- nothing below fails: the new store replaces the old one (whose memory goes with it); the counters go on
    R.device_chunks = c->world_store.device_chunks; R.host_chunks = c->world_store.host_chunks;
    for (size_t i = 0; i < ctxs.size(); i++) {
        (void)hipSetDevice(ctxs[i]->device);
        ctxs[i]->world_store = std::move(made[i]);
    }
    (void)hipSetDevice(c->device);
    return YCGE_OK;
}

// the records at `recs` (m of `bytes_each` bytes) on the current device, ws_pool_batch of them at a time: launch(device records, first, count)
template <class Launch>
static int pool_batches(ycge_ctx *c, const void *recs, size_t m, size_t bytes_each, DevBuf<uint8_t> &d_recs, const char *kernel, Launch launch)
{
    if (m == 0) return YCGE_OK;
    HIP_TRY(c, d_recs.alloc(m * bytes_each));
    HIP_TRY(c, hipMemcpy(d_recs.p, recs, m * bytes_each, hipMemcpyHostToDevice));
    const size_t per = (size_t)c->knobs.ws_pool_batch;
    for (size_t first = 0; first < m; first += per) {
        const int e = launch(d_recs.p + first * bytes_each, first, std::min(per, m - first));
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "%s launch failed: %s", kernel, hipGetErrorString((hipError_t)e));
    }
    return YCGE_OK;
}

// behind k_wp_planes on the root's stream: the part of every slot in use that lies in the x-planes [x0, x0 + planes) of a fields store, over the slab's cells (k_ws_pool_planes)
static int pool_into_slab(ycge_ctx *c, const WorldStore &st, int32_t x0, int32_t planes, int32_t *slab)
{
    if (!st.pool_used) return YCGE_OK;
    const WsShape &W = st.shape;
    std::vector<WsPoolPlanes> recs;
    for (int32_t slot = 0; slot < st.pool_cap; slot++) {
        const int32_t ci = st.chunk_in[(size_t)slot];
        if (ci < 0) continue;
        const int32_t cx = ci / (W.ncy * W.ncz), cy = ci / W.ncz % W.ncy, cz = ci % W.ncz;
        const int32_t lo = std::max(x0, cx * W.S), hi = std::min(x0 + planes, (cx + 1) * W.S);          // [lo, hi)
        if (lo >= hi) continue;
        recs.push_back(WsPoolPlanes{slot, lo - cx * W.S, hi - lo, lo - x0, cy, cz, {0, 0}});
    }
    DevBuf<uint8_t> d_recs;
    const int rc = pool_batches(c, recs.data(), recs.size(), sizeof(WsPoolPlanes), d_recs, "k_ws_pool_planes", [&](uint8_t *d, size_t, size_t m) {
        return ycge_launch_world_store_pool_planes(st.d_pool.p, st.pool_stride, W.S, (const WsPoolPlanes *)d, (int)m, slab, W.ny, W.nz, c->stream);
    });
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // (d_recs goes when this scope ends)
    return YCGE_OK;
}

int world_store_read(ycge_ctx *c, int32_t x0, int32_t planes, int32_t *cells_out)
{
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    const WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    const WsShape &W = st.shape;
    if (planes < 1 || x0 < 0 || x0 > W.nx - planes) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_read: planes [%d, %d + %d) of a world of %d", x0, x0, planes, W.nx);
    if (!cells_out) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_world_store_read: null cells_out");
    const size_t plane_cells = (size_t)W.ny * W.nz, plane_bytes = plane_cells * 8;
    if (st.on_host) { std::memcpy(cells_out, st.host_cells.data() + 2 * (size_t)x0 * plane_cells, (size_t)planes * plane_bytes); return YCGE_OK; }
    rc = quiesce(c);          // (copy_out's staging is the frames' too)
    if (rc != YCGE_OK) return rc;
    const DeviceGuard guard(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!st.fields) return copy_out(c, cells_out, st.d_cells.p + 2 * (size_t)x0 * plane_cells, (size_t)planes * plane_bytes);
    // a fields store: the planes are made in a device slab of their own, slab by slab, and copied out
    const size_t per = std::max<size_t>(1, std::min<size_t>((size_t)planes, c->knobs.world_store_slab_bytes / plane_bytes));
    DevBuf<int32_t> slab;
    HIP_TRY(c, slab.alloc(2 * per * plane_cells));
    WpFields F;
    wp_layout(st.d_fields.p, (size_t)W.nx * W.nz, 0, &F);
    for (size_t done = 0; done < (size_t)planes; done += per) {
        const size_t px = std::min(per, (size_t)planes - done);
        const int e = ycge_launch_worldpregen_planes(&st.gen_world, &st.gen_window, &F, (int32_t)((size_t)x0 + done), (int32_t)px, slab.p, c->stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_planes launch failed: %s", hipGetErrorString((hipError_t)e));
        rc = pool_into_slab(c, st, (int32_t)((size_t)x0 + done), (int32_t)px, slab.p);          // the edited chunks' cells over the generator's
        if (rc != YCGE_OK) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rc = copy_out(c, cells_out + 2 * done * plane_cells, slab.p, px * plane_bytes);
        if (rc != YCGE_OK) return rc;
    }
    return YCGE_OK;
}

// ycge_world_store_edit on a fields store with a pool (the ops checked already, one at least): copy-on-write at chunk granularity.
// Every chunk an op touches takes a slot - refused as a whole when the free slots do not suffice - and is made there by k_wp_fill, a
// launch per batch of chunks; the ops, clipped against the chunks they touch and sorted by slot, are applied by k_ws_pool_edit;
// k_ws_pool_occupied finds the touched slots' occupancy again and one read-back brings it home; the new slot map and occupancy are
// installed in a last step that cannot fail.  Every device of the context materialises and edits its own pool.
static int pool_edit(ycge_ctx *c, const std::vector<WsEditOp> &list)
{
    static const char *const fn = "ycge_world_store_edit";
    WorldStore &st = c->world_store;
    const WsShape &W = st.shape;
    const int S = W.S;
    auto chunks_of = [&](const WsEditOp &o, auto &&visit) {
        for (int cx = o.lo[0] / S; cx <= o.hi[0] / S; cx++)
            for (int cy = o.lo[1] / S; cy <= o.hi[1] / S; cy++)
                for (int cz = o.lo[2] / S; cz <= o.hi[2] / S; cz++) visit(cx, cy, cz);
    };
    // 1. the touched chunks that hold no slot yet, against the free slots
    const int32_t free_slots = st.pool_cap - st.pool_used;
    std::vector<uint8_t> counted(st.occupied.size(), 0);
    int64_t n_fresh = 0;
    int first_unfit = -1;
    for (size_t k = 0; k < list.size(); k++)
        chunks_of(list[k], [&](int cx, int cy, int cz) {
            const size_t ci = chunk_of(W, cx, cy, cz);
            if (st.slot_of[ci] >= 0 || counted[ci]) return;
            counted[ci] = 1;
            if (++n_fresh > free_slots && first_unfit < 0) first_unfit = (int)k;
        });
    if (first_unfit >= 0)
        return c->fail(YCGE_ERR_OUT_OF_MEMORY, "%s: op %d does not fit the edit pool: the ops touch %lld chunks that hold no slot and %d of its %d slots are free (ycge_world_store_reserve_edits grows the pool, ycge_world_store_revert_chunks gives slots back)",
                       fn, first_unfit, (long long)n_fresh, free_slots, st.pool_cap);
    // the new map, the chunks to make, the clipped ops and the touched slots - all on the host, nothing installed yet
    std::vector<int32_t> slot_of = st.slot_of, chunk_in = st.chunk_in;
    std::vector<int32_t> fresh_chunk, touched_slots;          // chunk numbers of the new slots, in the order they were given out; every slot an op touches, once
    std::vector<uint8_t> slot_touched((size_t)st.pool_cap, 0);
    std::vector<WsPoolEdit> recs;
    int32_t next_free = 0;
    for (const WsEditOp &o : list)
        chunks_of(o, [&](int cx, int cy, int cz) {
            const size_t ci = chunk_of(W, cx, cy, cz);
            if (slot_of[ci] < 0) {
                while (chunk_in[(size_t)next_free] >= 0) next_free++;          // (the lowest free slot: there is one, counted above)
                slot_of[ci] = next_free; chunk_in[(size_t)next_free] = (int32_t)ci;
                fresh_chunk.push_back((int32_t)ci);
            }
            const int32_t slot = slot_of[ci];
            if (!slot_touched[(size_t)slot]) { slot_touched[(size_t)slot] = 1; touched_slots.push_back(slot); }
            const int base[3] = {cx * S, cy * S, cz * S};
            WsPoolEdit r{};
            r.slot = slot; r.mat = o.mat; r.meta = o.meta;
            for (int a = 0; a < 3; a++) { r.lo[a] = std::max(o.lo[a] - base[a], 0); r.hi[a] = std::min(o.hi[a] - base[a], S - 1); }
            recs.push_back(r);
        });
    std::stable_sort(recs.begin(), recs.end(), [](const WsPoolEdit &a, const WsPoolEdit &b) { return a.slot < b.slot; });          // (list order stays inside a slot)
    const size_t m_fresh = fresh_chunk.size(), per = (size_t)c->knobs.ws_pool_batch;
    const size_t off_any = align_up(m_fresh * sizeof(WgChunk), 256);

    int rc = quiesce(c);          // (copy_out's staging is the frames' too)
    if (rc != YCGE_OK) return rc;
    const DeviceGuard guard(c->device);
    for (ycge_ctx *x : contexts_of(c)) {
        HIP_TRY(c, hipSetDevice(x->device));
        WorldStore &xs = x->world_store;
        // 2. the new slots' chunks, made where they will lie
        DevBuf<uint8_t> d_head, d_recs;
        if (m_fresh) {
            std::vector<uint8_t> head(off_any + m_fresh * sizeof(uint32_t), 0);          // the chunks' records, then their `any` words, zeroed (not read: step 4 finds the occupancy)
            for (size_t j = 0; j < m_fresh; j++) {
                const int32_t ci = fresh_chunk[j];
                ((WgChunk *)head.data())[j] = WgChunk{ci / (W.ncy * W.ncz), ci / W.ncz % W.ncy, ci % W.ncz, 0, (int32_t *)(xs.d_pool.p + (size_t)slot_of[(size_t)ci] * st.pool_stride)};
            }
            HIP_TRY(c, d_head.alloc(head.size()));
            HIP_TRY(c, hipMemcpy(d_head.p, head.data(), head.size(), hipMemcpyHostToDevice));
            WpFields F;
            wp_layout(xs.d_fields.p, (size_t)st.gen_window.nx * st.gen_window.nz, 0, &F);
            for (size_t first = 0; first < m_fresh; first += per) {
                const int e = ycge_launch_worldpregen_fill((const WgChunk *)d_head.p + first, (int)std::min(per, m_fresh - first), &st.gen_world, &st.gen_window, &F,
                                                           (uint32_t *)(d_head.p + off_any) + first, x->stream);
                if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_wp_fill launch failed: %s", hipGetErrorString((hipError_t)e));
            }
        }
        // 3. the ops
        rc = pool_batches(c, recs.data(), recs.size(), sizeof(WsPoolEdit), d_recs, "k_ws_pool_edit", [&](uint8_t *d, size_t first, size_t m) {
            uint64_t max_cells = 0;
            for (size_t k = first; k < first + m; k++) {
                const WsPoolEdit &r = recs[k];
                max_cells = std::max(max_cells, (uint64_t)(r.hi[0] - r.lo[0] + 1) * (uint64_t)(r.hi[1] - r.lo[1] + 1) * (uint64_t)(r.hi[2] - r.lo[2] + 1));
            }
            return ycge_launch_world_store_pool_edit(xs.d_pool.p, st.pool_stride, S, (const WsPoolEdit *)d, (int)m, max_cells, x->stream);
        });
        if (rc != YCGE_OK) return rc;
        HIP_TRY(c, hipStreamSynchronize(x->stream));          // (the records go when this scope ends)
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // 4. the touched slots' occupancy, on the root
    const size_t m_touched = touched_slots.size();
    std::vector<uint32_t> words(m_touched, 0);
    {
        DevBuf<uint8_t> d_slots;
        DevBuf<uint32_t> d_words;
        HIP_TRY(c, d_words.alloc(m_touched));
        HIP_TRY(c, hipMemsetAsync(d_words.p, 0, m_touched * 4, c->stream));
        rc = pool_batches(c, touched_slots.data(), m_touched, sizeof(int32_t), d_slots, "k_ws_pool_occupied", [&](uint8_t *d, size_t first, size_t m) {
            return ycge_launch_world_store_pool_occupied(st.d_pool.p, st.pool_stride, S, (const int32_t *)d, (int)m, d_words.p + first, c->stream);
        });
        if (rc != YCGE_OK) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rc = copy_out(c, words.data(), d_words.p, m_touched * 4);
        if (rc != YCGE_OK) return rc;
    }
    // 5. nothing below fails
    st.slot_of.swap(slot_of); st.chunk_in.swap(chunk_in);
    st.pool_used += (int32_t)m_fresh;
    for (size_t j = 0; j < m_touched; j++) st.occupied[(size_t)st.chunk_in[(size_t)touched_slots[j]]] = words[j] != 0;
    return YCGE_OK;
}

// ycge_world_store_edit: boxes of raw pairs written into the store where it lies, the later op winning; then the occupancy of the chunks
// the boxes touch, found again.  A device store: k_ws_edit on every device, launches of at most YCGE_WS_EDIT_OPS_PER_LAUNCH ops in list
// order on one stream (within a launch a lane leaves a cell to the last op that covers it); on the root the touched chunks' words are
// zeroed - the others keep what the store knows - and k_ws_occupied runs over the x-planes of every run of touched chunk columns.  A
// host store: two host loops.  Every refusal is decided before the first cell is written.
int world_store_edit(ycge_ctx *c, const ycge_voxel_edit *ops, int32_t n)
{
    static const char *const fn = "ycge_world_store_edit";
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    if (n < 0 || n > YCGE_VOXEL_EDIT_MAX_OPS || (n > 0 && !ops)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad op array (n = %d; at most %d ops)", fn, n, YCGE_VOXEL_EDIT_MAX_OPS);
    WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    if (st.fields && !st.pool_cap)
        return c->fail(YCGE_ERR_UNSUPPORTED, "%s: a fields store holds no cells to edit; generate the store with YCGE_WORLD_STORE_CELLS, or give this one a pool of materialised chunks (ycge_world_store_reserve_edits)", fn);
    const WsShape &W = st.shape;
    const int dims[3] = {W.nx, W.ny, W.nz};
    std::vector<WsEditOp> list((size_t)n);
    std::vector<uint8_t> touched(st.occupied.size(), 0);
    for (int k = 0; k < n; k++) {
        const ycge_voxel_edit &e = ops[k];
        if (e.grid_index != 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: grid_index %d (must be 0)", fn, k, e.grid_index);
        for (int a = 0; a < 3; a++) {
            if (e.lo[a] > e.hi[a]) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: lo %d > hi %d on axis %d", fn, k, e.lo[a], e.hi[a], a);
            if (e.lo[a] < 0 || e.hi[a] >= dims[a]) return c->fail(YCGE_ERR_INVALID_ARG, "%s: op %d: the box leaves the store (%d x %d x %d) on axis %d", fn, k, W.nx, W.ny, W.nz, a);
        }
        WsEditOp &o = list[(size_t)k];
        for (int a = 0; a < 3; a++) { o.lo[a] = e.lo[a]; o.hi[a] = e.hi[a]; }
        o.mat = e.mat_id; o.meta = e.meta_id;
        for (int cx = e.lo[0] / W.S; cx <= e.hi[0] / W.S; cx++)
            for (int cy = e.lo[1] / W.S; cy <= e.hi[1] / W.S; cy++)
                for (int cz = e.lo[2] / W.S; cz <= e.hi[2] / W.S; cz++) touched[chunk_of(W, cx, cy, cz)] = 1;
    }
    if (n == 0) return YCGE_OK;
    if (st.fields) return pool_edit(c, list);
    std::vector<uint8_t> occupied = st.occupied;          // (takes the store's place in a last step that cannot fail)
    const size_t per_cx = (size_t)W.ncy * W.ncz;

    if (st.on_host) {
        int32_t *cells = st.host_cells.data();
        for (const WsEditOp &o : list)
            for (size_t x = (size_t)o.lo[0]; x <= (size_t)o.hi[0]; x++)
                for (size_t y = (size_t)o.lo[1]; y <= (size_t)o.hi[1]; y++) {
                    int32_t *row = cells + 2 * ((x * W.ny + y) * W.nz);
                    for (size_t z = (size_t)o.lo[2]; z <= (size_t)o.hi[2]; z++) { row[2 * z] = o.mat; row[2 * z + 1] = o.meta; }
                }
        for (int cx = 0; cx < W.ncx; cx++)
            for (int cy = 0; cy < W.ncy; cy++)
                for (int cz = 0; cz < W.ncz; cz++) {
                    const size_t ci = chunk_of(W, cx, cy, cz);
                    if (!touched[ci]) continue;
                    int s[3];
                    clipped(W, cx, cy, cz, s);
                    const int32_t *base = cells + 2 * first_cell(W, cx, cy, cz);
                    uint8_t any = 0;
                    for (size_t lx = 0; lx < (size_t)s[0] && !any; lx++)
                        for (size_t ly = 0; ly < (size_t)s[1] && !any; ly++) {
                            const int32_t *row = base + 2 * ((lx * W.ny + ly) * W.nz);
                            for (size_t lz = 0; lz < (size_t)s[2]; lz++) if (row[2 * lz] != 0) { any = 1; break; }          // Item1 != 0, :716
                        }
                    occupied[ci] = any;
                }
        st.occupied.swap(occupied);
        return YCGE_OK;
    }

    rc = quiesce(c);          // (copy_out's staging is the frames' too)
    if (rc != YCGE_OK) return rc;
    const DeviceGuard guard(c->device);
    for (ycge_ctx *x : contexts_of(c)) {
        HIP_TRY(c, hipSetDevice(x->device));
        DevBuf<uint8_t> d_ops;
        HIP_TRY(c, d_ops.alloc((size_t)n * sizeof(WsEditOp)));
        HIP_TRY(c, hipMemcpy(d_ops.p, list.data(), (size_t)n * sizeof(WsEditOp), hipMemcpyHostToDevice));
        for (size_t first = 0; first < (size_t)n; first += YCGE_WS_EDIT_OPS_PER_LAUNCH) {
            const size_t m = std::min<size_t>(YCGE_WS_EDIT_OPS_PER_LAUNCH, (size_t)n - first);
            uint64_t max_cells = 0;
            for (size_t k = first; k < first + m; k++) {
                const WsEditOp &o = list[k];
                max_cells = std::max(max_cells, (uint64_t)(o.hi[0] - o.lo[0] + 1) * (uint64_t)(o.hi[1] - o.lo[1] + 1) * (uint64_t)(o.hi[2] - o.lo[2] + 1));
            }
            const int e = ycge_launch_world_store_edit(x->world_store.d_cells.p, &W, (const WsEditOp *)d_ops.p + first, (int)m, max_cells, x->stream);
            if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ws_edit launch failed: %s", hipGetErrorString((hipError_t)e));
        }
        HIP_TRY(c, hipStreamSynchronize(x->stream));          // (d_ops goes when this scope ends)
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the occupancy, on the root: a word per chunk of the touched chunk columns cx0..cx1, run by run
    for (int cx0 = 0; cx0 < W.ncx;) {
        auto column_touched = [&](int cx) { return std::find(touched.begin() + (ptrdiff_t)(cx * per_cx), touched.begin() + (ptrdiff_t)((cx + 1) * per_cx), (uint8_t)1) != touched.begin() + (ptrdiff_t)((cx + 1) * per_cx); };
        if (!column_touched(cx0)) { cx0++; continue; }
        int cx1 = cx0;
        while (cx1 + 1 < W.ncx && column_touched(cx1 + 1)) cx1++;
        const size_t first = (size_t)cx0 * per_cx, count = (size_t)(cx1 - cx0 + 1) * per_cx;
        std::vector<uint32_t> words(count);
        for (size_t i = 0; i < count; i++) words[i] = touched[first + i] ? 0u : (uint32_t)(occupied[first + i] != 0);
        DevBuf<uint32_t> d_occ;          // (as long as the whole store's: k_ws_occupied indexes it by the chunk's number)
        HIP_TRY(c, d_occ.alloc(st.occupied.size()));
        HIP_TRY(c, hipMemcpy(d_occ.p + first, words.data(), count * 4, hipMemcpyHostToDevice));
        const int x0 = cx0 * W.S, x1 = std::min(W.nx, (cx1 + 1) * W.S);
        const int e = ycge_launch_world_store_occupied(st.d_cells.p, &W, x0, x1 - x0, d_occ.p, c->stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ws_occupied launch failed: %s", hipGetErrorString((hipError_t)e));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        rc = copy_out(c, words.data(), d_occ.p + first, count * 4);
        if (rc != YCGE_OK) return rc;
        for (size_t i = 0; i < count; i++) occupied[first + i] = words[i] != 0;
        cx0 = cx1 + 1;
    }
    st.occupied.swap(occupied);
    return YCGE_OK;
}

// ycge_world_store_reserve_edits: the pool of a fields store made, or grown - every device's new pool allocated and the slots in use
// copied into it before any context takes its own, so a refusal or a failure leaves the store and an earlier pool as they were.
int world_store_reserve_edits(ycge_ctx *c, int32_t max_chunks)
{
    static const char *const fn = "ycge_world_store_reserve_edits";
    int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    if (!st.fields) return c->fail(YCGE_ERR_INVALID_ARG, "%s: the store is not in the fields form (YCGE_WORLD_STORE_FIELDS): it holds its cells and needs no pool", fn);
    const size_t n_chunks = st.occupied.size();
    if (max_chunks < 1 || (size_t)max_chunks > n_chunks) return c->fail(YCGE_ERR_INVALID_ARG, "%s: max_chunks %d is outside 1..%zu, the store's chunks", fn, max_chunks, n_chunks);
    if (max_chunks < st.pool_used) return c->fail(YCGE_ERR_INVALID_ARG, "%s: max_chunks %d is below the %d slots in use (ycge_world_store_revert_chunks gives slots back)", fn, max_chunks, st.pool_used);
    if (max_chunks == st.pool_cap) return YCGE_OK;
    const size_t S = (size_t)st.shape.S, stride = align_up(S * S * S * 8, 16);
    const std::vector<ycge_ctx *> ctxs = contexts_of(c);
    if (st.pool_cap) { rc = quiesce(c); if (rc != YCGE_OK) return rc; }          // (an attach in flight may read the old pool)
    const DeviceGuard guard(c->device);
    std::vector<DevBuf<uint8_t>> made(ctxs.size());
    // a smaller pool keeps its slots' numbers only while they fit: the slots in use are packed to the front of the new one
    std::vector<int32_t> slot_of(n_chunks, -1), chunk_in((size_t)max_chunks, -1);
    int32_t used = 0;
    for (int32_t slot = 0; slot < st.pool_cap; slot++) {
        const int32_t ci = st.chunk_in[(size_t)slot];
        if (ci < 0) continue;
        slot_of[(size_t)ci] = used; chunk_in[(size_t)used] = ci;
        used++;
    }
    for (size_t i = 0; i < ctxs.size(); i++) {
        HIP_TRY(c, hipSetDevice(ctxs[i]->device));
        HIP_TRY(c, made[i].alloc((size_t)max_chunks * stride));
        for (int32_t slot = 0; slot < st.pool_cap; slot++) {
            const int32_t ci = st.chunk_in[(size_t)slot];
            if (ci >= 0) HIP_TRY(c, hipMemcpyAsync(made[i].p + (size_t)slot_of[(size_t)ci] * stride, ctxs[i]->world_store.d_pool.p + (size_t)slot * stride, stride, hipMemcpyDeviceToDevice, ctxs[i]->stream));
        }
        HIP_TRY(c, hipStreamSynchronize(ctxs[i]->stream));
    }
    // ---- nothing below fails
    for (size_t i = 0; i < ctxs.size(); i++) {
        (void)hipSetDevice(ctxs[i]->device);
        ctxs[i]->world_store.d_pool = std::move(made[i]);
        ctxs[i]->world_store.pool_stride = stride;
    }
    (void)hipSetDevice(c->device);
    st.slot_of.swap(slot_of); st.chunk_in.swap(chunk_in);
    st.pool_cap = max_chunks; st.pool_used = used;
    return YCGE_OK;
}

int world_store_edit_slots(ycge_ctx *c, int32_t *capacity_out, int32_t *used_out)
{
    const int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    const WorldStore &st = c->world_store;
    if (capacity_out) *capacity_out = st.held ? st.pool_cap : 0;
    if (used_out) *used_out = st.held ? st.pool_used : 0;
    return YCGE_OK;
}

// ycge_world_store_revert_chunks: host work alone - a chunk without a slot is the generated chunk again to every reader
int world_store_revert_chunks(ycge_ctx *c, const int32_t *keys, int32_t n)
{
    static const char *const fn = "ycge_world_store_revert_chunks";
    const int rc = need_root(c);
    if (rc != YCGE_OK) return rc;
    if (n < 0 || (n > 0 && !keys)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad key array (n = %d)", fn, n);
    WorldStore &st = c->world_store;
    if (!st.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s", kNoStore);
    const WsShape &W = st.shape;
    for (int k = 0; k < n; k++) {
        const int32_t cx = keys[3 * k], cy = keys[3 * k + 1], cz = keys[3 * k + 2];
        if (cx < 0 || cy < 0 || cz < 0 || cx >= W.ncx || cy >= W.ncy || cz >= W.ncz)
            return c->fail(YCGE_ERR_INVALID_ARG, "%s: key %d: no chunk (%d, %d, %d) in a store of %d x %d x %d chunks", fn, k, cx, cy, cz, W.ncx, W.ncy, W.ncz);
    }
    if (!st.pool_cap) return YCGE_OK;
    for (int k = 0; k < n; k++) {
        const size_t ci = chunk_of(W, keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]);
        const int32_t slot = st.slot_of[ci];
        if (slot < 0) continue;
        st.slot_of[ci] = -1; st.chunk_in[(size_t)slot] = -1; st.pool_used--;
        st.occupied[ci] = st.gen_occupied[ci];
    }
    return YCGE_OK;
}

int world_store_generate_stats(ycge_ctx *c, int64_t *out9)
{
    if (!c || !out9) return YCGE_ERR_INVALID_ARG;
    const WorldStore &st = c->world_store;
    out9[0] = st.gen_form; out9[1] = st.gen_on_host; out9[2] = st.gen_passes; out9[3] = st.gen_slabs;
    for (int a = 0; a < 5; a++) out9[4 + a] = (int64_t)st.gen_us[a];
    return YCGE_OK;
}

}  // namespace ycge_host
