// ycge_worldgen_cells.h - the cell sources of generated chunks and the 2-D fields of a pregen window, shared by ycge_worldgen_scene.cpp
// (ycge_scene_generate_grids, ycge_scene_generate_world) and ycge_world_store.cpp (a world store whose source is the generator:
// ycge_world_store_generate).  One copy of the launch records, the fields' layout, the anyLeaves pass loop and the window's fill.
#pragma once
#include <algorithm>
#include <functional>

#include "ycge_ctx.h"
#include "ycge_grid_encode.h"
#include "ycge_worldgen_host.h"

namespace ycge_host {

constexpr size_t kGenGroupMax = 32768;               // chunks in one fill launch (gridDim.y)

// what the generators' sources share: the chunks' keys, the launch records of a fill and its time
struct GeneratedCells : CellSource {
    const char *fn, *kernel;                         // the export and its fill kernel, for the messages
    wg::World W;
    std::vector<std::array<int32_t, 3>> keys;        // per chunk
    std::vector<int32_t> col;                        // per chunk: its chunk column among the column records (k_wg_fill; k_wp_fill does not read it)
    double fill_us = 0;                              // the fill kernels on the root, all launches of the call
    GeneratedCells(const char *fn_, const char *kernel_, const wg::World &W_, bool device) : fn(fn_), kernel(kernel_), W(W_) { on_device = device; group_max = kGenGroupMax; }
    GeneratedCells(const char *fn_, const char *kernel_, const ycge_world *world, bool device) : GeneratedCells(fn_, kernel_, wg::make_world(world->chunk_size, world->chunks_y, world->world_seed), device) {}
    size_t chunk_bytes() const { return (size_t)W.size * W.size * W.size * 8; }
    size_t head_bytes(size_t m) const override { return align_up(m * sizeof(WgChunk), 256) + align_up(m * sizeof(uint32_t), 256); }
    virtual int launch(ycge_ctx *x, const WgChunk *chunks, int m, uint32_t *any_solid) = 0;
    // a chunk that came out otherwise than the export found before (solid: it holds something)
    int wrong(ycge_ctx *root, int k, bool solid) const { return root->fail(YCGE_ERR_INTERNAL, solid ? "%s: chunk (%d, %d, %d) came out empty" : "%s: chunk (%d, %d, %d) holds cells above its column's top", fn, keys[(size_t)k][0], keys[(size_t)k][1], keys[(size_t)k][2]); }
    // chunks ks[j] into d_cells[j] on x's stream: their records and zeroed `any` words at d_head, the launch; on the root also the wait, the time and the `any` words' verdict
    int fill_chunks(ycge_ctx *root, ycge_ctx *x, const std::vector<int> &ks, uint8_t *d_head, const std::vector<int32_t *> &d_cells, bool solid = true)
    {
        const size_t m = ks.size(), off_any = align_up(m * sizeof(WgChunk), 256);
        std::vector<uint8_t> head(GeneratedCells::head_bytes(m), 0);          // (its own part alone: a derived source may keep records of its own behind it)
        for (size_t j = 0; j < m; j++) { const auto &key = keys[(size_t)ks[j]]; ((WgChunk *)head.data())[j] = WgChunk{key[0], key[1], key[2], col[(size_t)ks[j]], d_cells[j]}; }
        HIP_TRY(root, hipMemcpy(d_head, head.data(), head.size(), hipMemcpyHostToDevice));
        const auto t0 = std::chrono::steady_clock::now();
        const int e = launch(x, (const WgChunk *)d_head, (int)m, (uint32_t *)(d_head + off_any));
        if (e != 0) return root->fail(YCGE_ERR_DEVICE, "%s launch failed: %s", kernel, hipGetErrorString((hipError_t)e));
        if (x != root) return YCGE_OK;
        HIP_TRY(root, hipStreamSynchronize(x->stream));
        fill_us += us_since(t0);
        std::vector<uint32_t> any(m);          // per chunk: != 0 when a cell is not Air
        const int rc = copy_out(root, any.data(), d_head + off_any, m * sizeof(uint32_t));
        for (size_t j = 0; j < m && rc == YCGE_OK; j++)
            if ((any[j] != 0) != solid) return wrong(root, ks[j], solid);
        return rc;
    }
};

// where the fields of a window of n columns (and the occupancy words of its n_chunks chunks, last: nothing else moves with their number)
// lie in an allocation that starts at `base`
inline size_t wp_layout(uint8_t *base, size_t n, size_t n_chunks, WpFields *F)
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
inline uint8_t *wp_next_flags(const WpFields &F, size_t n) { return F.fallback + align_up(n, 256); }

// The fields of window N made at `base` (wp_layout, on the current device) on `stream`: the 2-D field kernels, then the anyLeaves passes
// to their fixed point.  The root (is_root) decides the number of passes, reading the flip count back after each (`read_back`: a
// synchronous copy of device memory behind the stream), leaves it in `passes`, and then asks which chunks hold anything: `occupied`,
// one word per chunk.  A peer repeats `passes` passes and reads nothing back.  us: the field kernels, the pass loop, the occupancy
// kernel with its read-back (wall time, root only).  `c` takes the error text, `fn` names the export in it.  (ycge_worldgen_scene.cpp)
using WpReadBack = std::function<int(void *dst, const void *src, size_t bytes)>;
int wp_make_fields(ycge_ctx *c, const char *fn, bool is_root, uint8_t *base, const wg::World &W, const wg::Window &N, int chunks_y, int chunks_z, hipStream_t stream,
                   const WpReadBack &read_back, int &passes, double us[3], uint32_t *occupied);

// the chunks of a pregen window: keys are chunk coordinates in the window, one per grid of the attach.  The fields are those of
// ycge_scene_generate_world's call (x->d_wg_cols) unless a derived source keeps its own; host-made cells are slices of the whole world
// (never BESIDE the device: the export sends a large table there)
struct WindowCells : GeneratedCells {
    wg::Window N;
    int32_t *host_world = nullptr;                   // host: the whole world's cells, VG01 order
    int32_t *world_out = nullptr;                    // device: the caller's cells_out (whole world), or NULL
    WindowCells(const char *fn_, const wg::World &W_, bool device, wg::Window n) : GeneratedCells(fn_, "k_wp_fill", W_, device), N(n) {}
    WindowCells(const ycge_world *world, bool device, wg::Window n) : GeneratedCells("ycge_scene_generate_world", "k_wp_fill", world, device), N(n) {}
    virtual uint8_t *fields_of(ycge_ctx *x) const { return x->d_wg_cols.p; }
    // chunk `key` of a world in VG01 order <-> its S^3 cells in ycge_grid.cells order (rows of S cells along z): a slice of the world, or scattered into it
    void world_rows(const std::array<int32_t, 3> &key, int32_t *world, int32_t *chunk, bool scatter) const
    {
        const size_t S = (size_t)W.size, ny = (size_t)W.height, nz = (size_t)N.nz;
        for (size_t lx = 0; lx < S; lx++)
            for (size_t ly = 0; ly < S; ly++) {
                int32_t *w = world + 2 * (((key[0] * S + lx) * ny + key[1] * S + ly) * nz + key[2] * S), *r = chunk + 2 * (lx * S + ly) * S;
                std::memcpy(scatter ? w : r, scatter ? r : w, S * 8);
            }
    }
    int launch(ycge_ctx *x, const WgChunk *chunks, int m, uint32_t *any_solid) override
    {
        WpFields F;
        wp_layout(fields_of(x), (size_t)N.nx * N.nz, 0, &F);
        return ycge_launch_worldpregen_fill(chunks, m, &W, &N, &F, any_solid, x->stream);
    }
    int write(ycge_ctx *, size_t k, const ycge_grid &, int32_t *cells) override { world_rows(keys[k], host_world, cells, false); return YCGE_OK; }
    int fill(ycge_ctx *root, ycge_ctx *x, const std::vector<int> &group, uint8_t *d_head, const std::vector<int32_t *> &d_cells) override
    {
        int rc = fill_chunks(root, x, group, d_head, d_cells);
        if (rc != YCGE_OK || x != root || !world_out) return rc;
        std::vector<int32_t> made((size_t)(d_cells.back() - d_cells.front()) + chunk_bytes() / 4);          // the caller wants the cells: the group's cell area in ONE copy, scattered
        rc = copy_out(root, made.data(), d_cells.front(), made.size() * 4);
        for (size_t j = 0; j < group.size() && rc == YCGE_OK; j++) world_rows(keys[(size_t)group[j]], world_out, made.data() + (d_cells[j] - d_cells.front()), true);
        return rc;
    }
};

}  // namespace ycge_host
