// ycge_host.cpp - host side of the C-ABI in include/ycge.h: the context (creation, geometry and buffers, the order of its teardown), frame
// parameters, copy_out / quiesce, the RCCL loader, the exception barrier, camera / resize / frame counter, host buffers, the OBJ wrappers and
// the general test hooks (fault injection among them).  (Scene flattening, upload and updates: ycge_scene.cpp.  Mesh trees and the mesh arena:
// ycge_mesh_bvh.cpp.  Frame orchestration, frames in flight, the slab form of the tiled frame: ycge_frame.cpp.  The post stage:
// ycge_post_host.cpp.  The tile-resident multi-GPU form and the read-backs: ycge_resident.cpp.)
#include "ycge_ctx.h"
#include <dlfcn.h>

#ifndef YCGE_FAULT_INJECTION
#define YCGE_FAULT_INJECTION 0
#endif
#if YCGE_FAULT_INJECTION
#include <atomic>
#include <cstdlib>
#include <new>
static std::atomic<long long> g_fail_alloc_countdown{-1};      // < 0: off; n: the allocation n from now throws std::bad_alloc (ycge_debug_fail_allocation)
#endif
namespace ycge_host {

int alloc_frame_buffers(ycge_ctx *c)
{
    const size_t n = (size_t)c->hiW * c->hiH;
    HIP_TRY(c, c->current_hdr.alloc(3 * n)); HIP_TRY(c, c->g_albedo.alloc(3 * n)); HIP_TRY(c, c->g_normal.alloc(3 * n));
    HIP_TRY(c, c->g_depth.alloc(n)); HIP_TRY(c, c->sky.alloc(n));
    HIP_TRY(c, c->taa_hist.alloc(3 * n));
    guides_forget(c);           // (prev_* and the second set of guide planes: allocated by the frame forms that use them)
    HIP_TRY(c, hipMemset(c->taa_hist.p, 0, 3 * n * sizeof(float)));
    if (c->cfg.capture_debug) {
        HIP_TRY(c, c->dbg_rays.alloc(6 * n)); HIP_TRY(c, c->dbg_prim.alloc(n)); HIP_TRY(c, c->dbg_sub.alloc(n));
        HIP_TRY(c, c->dbg_hit_t.alloc(n)); HIP_TRY(c, c->dbg_rng.alloc(n));
    }
    HIP_TRY(c, c->counters.alloc(YCGE_COUNTER_WORDS));            // [0..4] SURVEY 8(d) counters of the counting instances (zeroed per frame), [8 + 8 i] lane steps of the timed instances (cumulative, spread over cache lines)
    HIP_TRY(c, hipMemset(c->counters.p, 0, YCGE_COUNTER_WORDS * sizeof(unsigned long long)));
    return YCGE_OK;
}

// queue segments, hit records and stack-spill columns: one 256-entry segment per owned tile
int alloc_tile_buffers(ycge_ctx *c)
{
    if (c->side_stream) { HIP_TRY(c, hipStreamSynchronize(c->side_stream)); c->order_pending = false; }      // schedule kernels of the old size
    const size_t lanes = (size_t)(c->n_owned > 0 ? c->n_owned : 1) * 256;
    const size_t stack_lanes = lanes * YCGE_SCHEDULE_SLACK;      // k_trace's grid includes the schedule's slack entries
    HIP_TRY(c, c->wf_q0.alloc(lanes * ycge_wf_sizes(0))); HIP_TRY(c, c->wf_q1.alloc(lanes * ycge_wf_sizes(0)));
    HIP_TRY(c, c->wf_hit.alloc(lanes * ycge_wf_sizes(1))); HIP_TRY(c, c->wf_lq.alloc(lanes * ycge_wf_sizes(2)));
    HIP_TRY(c, c->wf_seg.alloc(4));
    HIP_TRY(c, c->wf_counts.alloc((size_t)(c->n_owned > 0 ? c->n_owned : 1) * 8));
    HIP_TRY(c, c->stack_spill.alloc((size_t)(c->spill_levels > 0 ? c->spill_levels : 1) * stack_lanes));
    c->stack_spill2.release(); c->stack_spill_side.release(); c->stack_spill_side2.release();
    c->wf2_q0.release(); c->wf2_q1.release(); c->wf2_hit.release(); c->wf2_lq.release(); c->wf2_seg.release(); c->wf2_counts.release();
    c->path_stack.release();
   
    {
        const size_t nb = (size_t)(c->n_owned > 0 ? c->n_owned : 1) * 4;
        HIP_TRY(c, c->block_cost.alloc(nb * YCGE_COST_FRAMES)); HIP_TRY(c, c->block_order.alloc(nb * YCGE_SCHEDULE_SLACK)); HIP_TRY(c, c->order_ws.alloc(96));
        HIP_TRY(c, c->cost_snap.alloc(nb * (ycge_ctx::kResCostFrames > YCGE_COST_FRAMES ? ycge_ctx::kResCostFrames : YCGE_COST_FRAMES)));
        HIP_TRY(c, hipMemset(c->order_ws.p, 0, 96 * sizeof(uint32_t)));
        HIP_TRY(c, hipMemset(c->block_cost.p, 0, nb * YCGE_COST_FRAMES * sizeof(uint32_t)));
        c->block_order_valid = false;
        for (int k = 0; k < 3; k++) { c->flight_order[k].release(); c->flight_ws[k].release(); c->flight_order_frame[k] = -1; }      // (allocated by the first frame in flight)
    }
    {   // XCD-aware block -> tile table: bucket the owned tiles by image strip (4 tiles = 128 px wide, strip s -> XCD s % 8),
        // then deal the buckets out round-robin so that block b (which lands on XCD b % 8) draws from bucket b % 8
        const int n = c->n_owned, world = c->cfg.world_size, rank = c->cfg.rank;
        std::vector<std::vector<uint32_t>> bucket(8);
        for (int k = 0; k < n; k++) {
            const int tile_id = rank + k * world;
            bucket[((tile_id % c->tiles_x) / 4) % 8].push_back((uint32_t)k);
        }
        std::vector<uint32_t> order;
        order.reserve(n > 0 ? n : 1);
        size_t pos[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int b = 0; (int)order.size() < n; b++) {
            int x = b % 8;
            if (pos[x] >= bucket[x].size()) {          // bucket exhausted: borrow from the fullest one
                size_t best = 0; int bi = -1;
                for (int y = 0; y < 8; y++) { const size_t left = bucket[y].size() - pos[y]; if (left > best) { best = left; bi = y; } }
                x = bi;
            }
            order.push_back(bucket[x][pos[x]++]);
        }
        if (order.empty()) order.push_back(0);
        HIP_TRY(c, c->tile_order.upload(order));
    }
    return YCGE_OK;
}

// ---- tile-resident form: halo lists.  Rank r needs {hdr, sky} of the one-pixel ring around each of its tiles (TAA's 3x3 window,
// TemporalBlendWithClamp clampRadius = 1, RaytraceRenderer.cs:218) from the ranks that own those pixels.  Both sides enumerate the ring
// pixels of the RECEIVER's tiles - tiles ascending; per tile the row above (x0 - 1 .. x0 + 32), the row below, the column left (y0 .. y0 + 7),
// the column right; pixels outside the image do not exist (TAA clamps its taps to the image) - and keep those the SENDER owns: the k-th such
// pixel is the k-th record of the (sender -> receiver) segment.  A pixel that borders two tiles of the receiver appears twice.  The same
// arithmetic in numpy: yetanotherconsolegameengine_amd/tiles.py (halo_lists); the CPU tests hold the two to each other.
static void halo_ring_of(int tile, int tiles_x, int hiW, int hiH, std::vector<uint32_t> &px)
{
    const int x0 = (tile % tiles_x) * YCGE_TILE_W, y0 = (tile / tiles_x) * YCGE_TILE_H;
    auto add = [&](int x, int y) { if (x >= 0 && y >= 0 && x < hiW && y < hiH) px.push_back((uint32_t)x + (uint32_t)y * (uint32_t)hiW); };
    for (int x = x0 - 1; x <= x0 + YCGE_TILE_W; x++) add(x, y0 - 1);
    for (int x = x0 - 1; x <= x0 + YCGE_TILE_W; x++) add(x, y0 + YCGE_TILE_H);
    for (int y = y0; y < y0 + YCGE_TILE_H; y++) add(x0 - 1, y);
    for (int y = y0; y < y0 + YCGE_TILE_H; y++) add(x0 + YCGE_TILE_W, y);
}
// send_px: pixels this rank gathers, segment by destination rank ascending; recv_px: pixels the received records scatter to, by source rank ascending
void halo_layout(int hiW, int hiH, int rank, int world, std::vector<int64_t> &send_counts, std::vector<int64_t> &recv_counts, std::vector<uint32_t> &send_px, std::vector<uint32_t> &recv_px)
{
    const int tiles_x = (hiW + YCGE_TILE_W - 1) / YCGE_TILE_W, tiles_y = (hiH + YCGE_TILE_H - 1) / YCGE_TILE_H, n_tiles = tiles_x * tiles_y;
    auto owner = [&](uint32_t p) { const int x = (int)(p % (uint32_t)hiW), y = (int)(p / (uint32_t)hiW); return ((y / YCGE_TILE_H) * tiles_x + x / YCGE_TILE_W) % world; };
    send_counts.assign((size_t)world, 0); recv_counts.assign((size_t)world, 0);
    send_px.clear(); recv_px.clear();
    std::vector<uint32_t> ring;
    std::vector<std::vector<uint32_t>> from((size_t)world);
    for (int t = rank; t < n_tiles; t += world) {          // what I receive: the ring of MY tiles, by owner
        ring.clear(); halo_ring_of(t, tiles_x, hiW, hiH, ring);
        for (uint32_t p : ring) { const int q = owner(p); if (q != rank) from[(size_t)q].push_back(p); }
    }
    for (int q = 0; q < world; q++) { recv_counts[(size_t)q] = (int64_t)from[(size_t)q].size(); recv_px.insert(recv_px.end(), from[(size_t)q].begin(), from[(size_t)q].end()); }
    for (int r = 0; r < world; r++) {                      // what I send: the ring of rank r's tiles, the pixels I own
        if (r == rank) continue;
        for (int t = r; t < n_tiles; t += world) {
            ring.clear(); halo_ring_of(t, tiles_x, hiW, hiH, ring);
            for (uint32_t p : ring) if (owner(p) == rank) { send_px.push_back(p); send_counts[(size_t)r]++; }
        }
    }
}
// the ring of the tile-resident form, its schedules and halo lists: all per size (callers have quiesced the device)
void release_resident(ycge_ctx *c)
{
    c->rsets.clear();
    c->res_order.clear(); c->res_ws.clear();
    c->res_order_ev.clear(); c->res_order_read_ev.clear(); c->res_order_frame.clear();
    c->res_last_traced.release(); c->res_last_traced_used = false;
    c->res_cost.release(); c->d_halo_send_px.release(); c->d_halo_recv_px.release(); c->d_halo_index.release();
    c->halo_send_counts.clear(); c->halo_recv_counts.clear(); c->halo_ready = false;
}

// floats per slab pixel: hdr, [albedo,] normal, depth, sky
size_t slab_floats(const ycge_ctx *c) { return c->cfg.slab_albedo ? (size_t)YCGE_SLAB_FLOATS : (size_t)YCGE_SLAB_FLOATS - 3; }

int set_geometry(ycge_ctx *c, int fbw, int fbh, int ss)
{
    if (fbw <= 0 || fbh <= 0) return c->fail(YCGE_ERR_INVALID_ARG, "framebuffer size must be positive");
    c->fbW = fbw; c->fbH = fbh; c->ss = ss < 1 ? 1 : ss;        // Math.Max(1, superSample), RaytraceRenderer.cs:81
    c->hiW = c->fbW * c->ss; c->hiH = c->fbH * 2 * c->ss;      // :86-87
    c->tiles_x = (c->hiW + YCGE_TILE_W - 1) / YCGE_TILE_W;
    c->tiles_y = (c->hiH + YCGE_TILE_H - 1) / YCGE_TILE_H;
    c->n_tiles = c->tiles_x * c->tiles_y;
    const int world = c->cfg.world_size, rank = c->cfg.rank;
    c->n_owned = rank < c->n_tiles ? (c->n_tiles - rank + world - 1) / world : 0;
    c->tiles_per_rank_padded = (c->n_tiles + world - 1) / world;
    c->taa_valid = false;                                       // Resize: taaHistoryValid = false (:137), taa.Resize (TemporalAA.cs:34-46)
    c->last_cam[0] = c->last_cam[1] = c->last_cam[2] = NAN; c->last_yaw = c->last_pitch = NAN;
    c->den_a.release(); c->den_b.release(); c->unit_n.release(); c->exp_terms.release(); c->exp_scratch.release(); c->d_sdr.release(); c->d_sdr2.release(); c->atrous_statw.release();     // spatialA / spatialB, :129-130
    c->chexels.out[0].release(); c->chexels.out[1].release(); c->chexels.ansi_stream.release(); c->chexels.ansi_tiles.release();      // (the encoded chexels and their stream: sized for the console)
    c->chexels.delta_held[0].release(); c->chexels.delta_held[1].release(); c->chexels.delta_valid = false;      // (the next delta call, of either colour form, returns a keyframe)
    c->denoised = nullptr;
    c->alt_post.release();
    c->wave_prof.release();                                     // sized for the tile grid
    c->pending.clear();
    c->t_hdr.release(); c->t_albedo.release(); c->t_normal.release(); c->t_depth.release(); c->t_sky.release();
    c->alt_hdr.release(); c->alt_albedo.release(); c->alt_normal.release(); c->alt_depth.release(); c->alt_sky.release();      // (callers have quiesced the device)
    c->alt2_hdr.release(); c->alt2_albedo.release(); c->alt2_normal.release(); c->alt2_depth.release(); c->alt2_sky.release();
    c->set_read[0] = c->set_read[1] = c->set_read[2] = false; c->out_set = 0; c->async_outstanding = false;
    c->tile_trace_used[0] = c->tile_trace_used[1] = false;
    release_resident(c);                                        // the ring of the tile-resident form and its halo lists are per size
    c->schedules.clear();                         // level schedules are per size: rebuilt on demand
    int rc = alloc_frame_buffers(c);
    if (rc != YCGE_OK) return rc;
    rc = alloc_tile_buffers(c);
    if (rc != YCGE_OK) return rc;
    const bool rccl_frame = c->cfg.multi_device_exchange == YCGE_EXCHANGE_RCCL;      // (ycge_create leaves the field set only on the contexts of a one-process multi-device frame)
    if (world > 1 || rccl_frame) HIP_TRY(c, c->own_slab.alloc((size_t)c->tiles_per_rank_padded * 256 * slab_floats(c)));
    if (rccl_frame) HIP_TRY(c, c->all_slabs.alloc((size_t)world * c->tiles_per_rank_padded * 256 * slab_floats(c))); else c->all_slabs.release();
    return YCGE_OK;
}

bool should_reset_history(const ycge_ctx *c, const float pos[3], float yaw, float pitch)   // TemporalAA.cs:58-67
{
    float dx = pos[0] - c->last_cam[0], dy = pos[1] - c->last_cam[1], dz = pos[2] - c->last_cam[2];
    float trans = is_nan(dx) ? 0.0f : cs_sqrt(dx * dx + dy * dy + dz * dz);
    float dyaw = is_nan(c->last_yaw) ? 0.0f : cs_abs(yaw - c->last_yaw);
    float dpitch = is_nan(c->last_pitch) ? 0.0f : cs_abs(pitch - c->last_pitch);
    return trans > c->cfg.motion_trans_reset || dyaw > c->cfg.motion_rot_reset || dpitch > c->cfg.motion_rot_reset;
}

H3 h_norm(H3 a)
{
    float l = a.x * a.x + a.y * a.y + a.z * a.z;
    if (l <= 0.0f) return a;
    float inv = 1.0f / cs_sqrt(l);
    return H3{a.x * inv, a.y * inv, a.z * inv};
}
H3 h_cross(H3 a, H3 b) { return H3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// per-frame constants of MakeJitteredRay (RaytraceRenderer.cs:413-434): host-side sin/cos/tan, as in the C#
void fill_frame_params(ycge_ctx *c, FrameParams &P, int64_t frame, const float pos[3], float yaw, float pitch, float fov_deg)
{
    std::memset(&P, 0, sizeof P);
    P.hiW = c->hiW; P.hiH = c->hiH;
    P.frame = frame;
    P.frame_idx = (int)(frame & 0x7fffffff);
    auto fracf = [](float v) { return v - cs_floor(v); };
    P.rot_x = fracf((float)(P.frame_idx + 1) * 0.61803398875f);
    P.rot_y = fracf((float)(P.frame_idx + 1) * 0.38196601125f);
    const float aspect = (float)c->hiW / (float)c->hiH;
    const float pi = 3.14159265358979323846f;
    float cp = cosf(pitch);
    H3 f = H3{sinf(yaw) * cp, sinf(pitch), -cosf(yaw) * cp};
    float fov_rad = fov_deg * (pi / 180.0f);
    P.half_h = tanf(0.5f * fov_rad);
    P.half_w = P.half_h * aspect;
    H3 fwd = h_norm(f);
    H3 right = h_norm(h_cross(fwd, H3{0.0f, 1.0f, 0.0f}));
    H3 up = h_norm(h_cross(right, fwd));
    P.cam_pos[0] = pos[0]; P.cam_pos[1] = pos[1]; P.cam_pos[2] = pos[2];
    P.fwd[0] = fwd.x; P.fwd[1] = fwd.y; P.fwd[2] = fwd.z;
    P.right[0] = right.x; P.right[1] = right.y; P.right[2] = right.z;
    P.up[0] = up.x; P.up[1] = up.y; P.up[2] = up.z;
    P.seed_salt = c->cfg.seed_salt;
    P.eps = c->cfg.eps;
    P.mirror_threshold = c->cfg.mirror_threshold;
    P.sigma_rad = c->cfg.diffuse_sigma_deg * (pi / 180.0f);
    {   // OrenNayarBRDF's sigma-only terms, same fp32 expressions as RaytraceRenderer.cs:823-825
        const float sigma2 = P.sigma_rad * P.sigma_rad;
        P.on_a = 1.0f - (sigma2 / (2.0f * (sigma2 + 0.33f)));
        P.on_b = 0.45f * sigma2 / (sigma2 + 0.09f);
    }
    P.max_mirror_bounces = c->cfg.max_mirror_bounces;
    P.max_refractions = c->cfg.max_refractions;
    P.diffuse_bounces = c->cfg.diffuse_bounces;
    P.tiles_x = c->tiles_x; P.tiles_y = c->tiles_y;
    P.rank = c->cfg.rank; P.world_size = c->cfg.world_size;
    P.n_owned_tiles = c->n_owned;
    // measured on config 4: strip-per-XCD ordering is 2.1x SLOWER than plain round-robin (1.79 vs 0.84 ms): the
    // heavy tiles cluster in a few strips and the frame is bounded by its heaviest tiles, so spreading them over
    // all 8 XCDs beats L2 affinity.  Kept as an opt-in experiment knob only.
    P.tile_order = c->knobs.xcd_strips ? c->tile_order.p : nullptr;
}

int morton3(int x, int y, int z)
{
    return ((x & 1) << 0) | ((y & 1) << 1) | ((z & 1) << 2) | ((x & 2) << 2) | ((y & 2) << 3) | ((z & 2) << 4) | ((x & 4) << 4) | ((y & 4) << 5) | ((z & 4) << 6);
}

static RcclApi g_rccl;
const RcclApi &load_rccl()
{
    static std::mutex m;
    std::lock_guard<std::mutex> g(m);
    if (g_rccl.tried) return g_rccl;
    g_rccl.tried = true;
    const char *forced = getenv("YCGE_RCCL_LIB");             // (tests: a name that does not exist = "RCCL absent")
    const char *names[] = {forced ? forced : "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (int pass = 0; pass < 2 && !g_rccl.h; pass++)
        for (const char *n : names) {
            g_rccl.h = dlopen(n, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
            if (g_rccl.h || forced) break;
        }
    if (!g_rccl.h) return g_rccl;
    auto sym = [&](const char *n) { return dlsym(g_rccl.h, n); };
    g_rccl.CommInitAll = (int (*)(void **, int, const int *))sym("ncclCommInitAll");
    g_rccl.CommDestroy = (int (*)(void *))sym("ncclCommDestroy");
    g_rccl.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))sym("ncclAllGather");
    g_rccl.GroupStart = (int (*)())sym("ncclGroupStart");
    g_rccl.GroupEnd = (int (*)())sym("ncclGroupEnd");
    g_rccl.GetErrorString = (const char *(*)(int))sym("ncclGetErrorString");
    g_rccl.ok = g_rccl.CommInitAll && g_rccl.CommDestroy && g_rccl.AllGather && g_rccl.GroupStart && g_rccl.GroupEnd;
    return g_rccl;
}

int abi_catch(const ycge_ctx *cc) noexcept
{
    ycge_ctx *c = const_cast<ycge_ctx *>(cc);
    int code = YCGE_ERR_INTERNAL;
    char text[320];
    std::snprintf(text, sizeof text, "internal error: unknown C++ exception stopped at the C-ABI");
    try { throw; }
    catch (const std::bad_alloc &) { code = YCGE_ERR_OUT_OF_MEMORY; std::snprintf(text, sizeof text, "out of host memory (std::bad_alloc stopped at the C-ABI)"); }
    catch (const std::exception &e) { std::snprintf(text, sizeof text, "internal error: %s (C++ exception stopped at the C-ABI)", e.what()); }
    catch (...) { }
    try { if (c) c->err = text; else g_create_error = text; } catch (...) { }      // (the message itself may not fit any more: the code still says what happened)
    return code;
}

} // namespace ycge_host

// =========================================================================== C-ABI
extern "C" {

int ycge_config_default(ycge_config *cfg)
try {
    if (!cfg) return YCGE_ERR_INVALID_ARG;
    std::memset(cfg, 0, sizeof *cfg);
    cfg->abi_version = YCGE_ABI_VERSION;
    cfg->slab_albedo = 1; cfg->n_devices = 0;
    cfg->atrous_inplace_exact = 1;
    cfg->tile_ring = 0;
    cfg->multi_device_exchange = YCGE_EXCHANGE_PEER_PUSH;
    cfg->fb_width = 80; cfg->fb_height = 45; cfg->super_sample = 1;
    cfg->fov_deg = 45.0f;
    cfg->device = 0; cfg->rank = 0; cfg->world_size = 1;
    cfg->diffuse_bounces = 1; cfg->max_mirror_bounces = 2; cfg->max_refractions = 2;
    cfg->mirror_threshold = 0.9f; cfg->eps = 1e-4f;
    cfg->seed_salt = 0x9E3779B97F4A7C15ULL;
    cfg->taa_alpha = 0.01f; cfg->motion_trans_reset = 0.0025f; cfg->motion_rot_reset = 0.0025f;
    cfg->diffuse_sigma_deg = 25.0f;
    cfg->taa_clamp_radius = 1; cfg->taa_luminance_pad = 0.10f;
    cfg->atrous_iterations = 3; cfg->atrous_c_phi = 3.0f; cfg->atrous_n_phi = 0.35f; cfg->atrous_z_phi = 2.0f; cfg->atrous_a_phi = 0.20f;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

static int create_one(const ycge_config *cfg, ycge_ctx *parent, ycge_ctx **out)
{
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        g_create_error = "no HIP device: the ray-trace path has no CPU fallback";
        return YCGE_ERR_NO_DEVICE_CODE;
    }
    if (cfg->device < 0 || cfg->device >= n_dev) { g_create_error = "device ordinal out of range"; return YCGE_ERR_INVALID_ARG; }
    std::unique_ptr<ycge_ctx> c(new ycge_ctx());      // (whatever way out of this function, an exception included, takes the context and its streams with it)
    c->err.reserve(320);
    c->cfg = *cfg;
    c->device = cfg->device;
    c->fov_deg = cfg->fov_deg;
    c->parent = parent;
    c->knobs.read();                // every YCGE_* knob is read here, once
    auto bail = [&](int code, const char *what = nullptr) { if (what) c->err = what; g_create_error = c->err; return code; };
    if (hipSetDevice(c->device) != hipSuccess) return bail(YCGE_ERR_DEVICE, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) return bail(YCGE_ERR_DEVICE, "hipGetDeviceProperties failed");
    std::snprintf(c->device_name, sizeof c->device_name, "%s (%s)", prop.name, prop.gcnArchName);
    c->compute_units = prop.multiProcessorCount;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        c->err = std::string("device is ") + prop.gcnArchName + "; this library carries gfx950 code only";
        return bail(YCGE_ERR_NO_DEVICE_CODE);
    }
    if (c->stream.ensure() != hipSuccess) return bail(YCGE_ERR_DEVICE, "stream creation failed");
    for (Event &ev : c->ev)
        if (ev.ensure(hipEventDefault) != hipSuccess) return bail(YCGE_ERR_DEVICE, "event creation failed");
    {
        if (c->side_stream.ensure() != hipSuccess) return bail(YCGE_ERR_DEVICE, "stream creation failed");
        if (c->cfg.world_size == 1 && c->cfg.n_devices <= 1) {
            // The second stream of the frames in flight (ycge_render_frame_async), created HERE, next to the other two: the runtime deals
            // streams onto a few hardware queues in order of creation, and a stream created later - after another context of the process
            // has come and gone - landed on the queue of this context's own stream: TAA and trace in ONE queue, 0.65 instead of 0.53 ms
            // a frame on config 4.  At the LOWEST priority: its kernels - TAA of the frame just traced, the schedule of the frame after
            // next - yield to the running trace's workgroups (measured neutral: 0.548 against 0.551 ms at normal priority)
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
                c->taa_stream.ensure_with_priority(c->knobs.flight_priority > 0 ? hi : c->knobs.flight_priority < 0 ? lo : 0) != hipSuccess ||
                c->stream2.ensure() != hipSuccess ||
                c->flight_fork_ev.ensure() != hipSuccess) return bail(YCGE_ERR_DEVICE, "stream creation failed");
        }
        for (Event *ev : {&c->side_ev[0], &c->side_ev[1], &c->traced_ev, &c->order_ev, &c->pushed_ev})
            if (ev->ensure() != hipSuccess) return bail(YCGE_ERR_DEVICE, "event creation failed");
    }
    int rc = set_geometry(c.get(), cfg->fb_width, cfg->fb_height, cfg->super_sample);
    if (rc != YCGE_OK) return bail(rc);
    *out = c.release();
    return YCGE_OK;
}

int ycge_create(const ycge_config *cfg, ycge_ctx **out)
try {
    if (!cfg || !out) { g_create_error = "null argument"; return YCGE_ERR_INVALID_ARG; }
    *out = nullptr;
    if (cfg->abi_version != YCGE_ABI_VERSION) { g_create_error = "abi_version mismatch"; return YCGE_ERR_INVALID_ARG; }
    if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) { g_create_error = "bad rank/world_size"; return YCGE_ERR_INVALID_ARG; }
    // the kernels implement the reference's compile-time constants (RaytraceRenderer.cs:31-36): in particular the path stack is
    // sized for MaxMirrorBounces = 2 (at most 3 live items), so any other value is refused here instead of dropping items
    if (cfg->diffuse_bounces != 1 || cfg->max_mirror_bounces != 2 || cfg->max_refractions != 2 || cfg->taa_clamp_radius < 0) {
        g_create_error = "DiffuseBounces/MaxMirrorBounces/MaxRefractions are compile-time constants in the reference (1/2/2)";
        return YCGE_ERR_UNSUPPORTED;
    }
    if (cfg->n_devices < 0 || cfg->n_devices > YCGE_MAX_DEVICES) { g_create_error = "n_devices out of range"; return YCGE_ERR_INVALID_ARG; }
    if (cfg->multi_device_exchange != YCGE_EXCHANGE_PEER_PUSH && cfg->multi_device_exchange != YCGE_EXCHANGE_RCCL) { g_create_error = "multi_device_exchange: unknown mode"; return YCGE_ERR_INVALID_ARG; }
    // the collective behind the one call (ABI 9): asked for, with a device list, and librccl.so there - else the peers push their tiles as before
    const bool want_rccl = cfg->multi_device_exchange == YCGE_EXCHANGE_RCCL && cfg->n_devices >= 1 && cfg->world_size == 1 && load_rccl().ok;
    if (cfg->n_devices <= 1 && !want_rccl) {
        ycge_config one = *cfg;
        if (cfg->n_devices == 1) one.device = cfg->devices[0];
        one.n_devices = 0;
        one.multi_device_exchange = YCGE_EXCHANGE_PEER_PUSH;
        return create_one(&one, nullptr, out);
    }
    // ---- one process, n_devices GPUs: this context is rank 0 on devices[0]; ranks 1.. live in peer contexts it owns
    if (cfg->world_size != 1 || cfg->rank != 0) { g_create_error = "n_devices > 1 excludes rank/world_size (that is the one-process-per-GPU form)"; return YCGE_ERR_INVALID_ARG; }
    ycge_config base = *cfg;
    base.world_size = cfg->n_devices; base.n_devices = 0;
    base.rank = 0; base.device = cfg->devices[0];
    base.multi_device_exchange = want_rccl ? YCGE_EXCHANGE_RCCL : YCGE_EXCHANGE_PEER_PUSH;
    if (want_rccl)
        for (int a = 0; a < cfg->n_devices; a++)
            for (int b = a + 1; b < cfg->n_devices; b++)
                if (cfg->devices[a] == cfg->devices[b]) { g_create_error = "multi_device_exchange = RCCL needs distinct devices (RCCL refuses two ranks on one GPU)"; return YCGE_ERR_INVALID_ARG; }
    ycge_ctx *root = nullptr;
    int rc = create_one(&base, nullptr, &root);
    if (rc != YCGE_OK) return rc;
    // (whatever throws below - a vector that grows, a thread that cannot start - takes the root, its peers and their threads with it)
    std::unique_ptr<ycge_ctx> owner(root);
    root->cfg.n_devices = cfg->n_devices;
    root->peers.reserve((size_t)cfg->n_devices);
    for (int r = 1; r < cfg->n_devices; r++) {
        ycge_config pc = base;
        pc.rank = r; pc.device = cfg->devices[r];
        ycge_ctx *peer = nullptr;
        rc = create_one(&pc, root, &peer);
        if (rc != YCGE_OK) return rc;
        root->peers.push_back(peer);              // (room was reserved: the root owns it from here)
        if (peer->device != root->device) {        // the peer's kernels write into the root's frame buffers over xGMI
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, peer->device, root->device) != hipSuccess || !can) {
                g_create_error = "devices cannot access each other's memory (no xGMI / PCIe peer path)";
                return YCGE_ERR_DEVICE;
            }
            (void)hipSetDevice(peer->device);
            const hipError_t pe = hipDeviceEnablePeerAccess(root->device, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) { g_create_error = "hipDeviceEnablePeerAccess failed"; return YCGE_ERR_DEVICE; }
            (void)hipGetLastError();
        }
    }
    if (want_rccl) {            // one communicator per device, all in this process (ncclCommInitAll); rank r = devices[r]
        const RcclApi &R = load_rccl();
        root->nccl_comms.assign((size_t)cfg->n_devices, nullptr);
        const int nr = R.CommInitAll(root->nccl_comms.data(), cfg->n_devices, cfg->devices);
        if (nr != 0) {
            g_create_error = std::string("ncclCommInitAll failed: ") + (R.GetErrorString ? R.GetErrorString(nr) : "?");
            root->nccl_comms.clear();
            return YCGE_ERR_DEVICE;
        }
        root->exchange_mode = YCGE_EXCHANGE_RCCL;
        (void)hipSetDevice(root->device);
    }
    for (ycge_ctx *peer : root->peers) {        // each peer's share of a frame is issued by its own thread (trace_on_all_devices)
        peer->worker.reset(new ycge_ctx::PeerWorker);
        peer->worker->th = std::thread(ycge_peer_worker_main, root, peer);
    }
    (void)hipSetDevice(root->device);
    *out = owner.release();
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

void ycge_destroy(ycge_ctx *c)
try {
    if (c) delete c;
}
catch (...) { (void)ycge_host::abi_catch(nullptr); }

} // extern "C"

void ycge_ctx::stop_worker()
{
    if (!worker) return;
    { std::lock_guard<std::mutex> g(worker->m); worker->job = -1; }
    worker->cv.notify_all();
    if (worker->th.joinable()) worker->th.join();
    worker.reset();
}

// frames in flight may still be on ANY of the context's streams (TAA, post stage and read-back on taa_stream / stream2; a query on its own)
void ycge_ctx::drain()
{
    (void)hipSetDevice(device);
    for (hipStream_t s : {(hipStream_t)side_stream, (hipStream_t)stream, (hipStream_t)taa_stream, (hipStream_t)stream2, query ? (hipStream_t)query->stream : nullptr})
        if (s) (void)hipStreamSynchronize(s);
}

// The body holds what has an ORDER; everything else goes with the members, each through its owner.  Nothing here relies on the order the
// members are declared in: when the body is done no thread issues work for this context, no communicator exists and every stream of every
// rank is idle, so buffers, events and streams may go in any order (and a member added tomorrow needs no line here).
//   1. the thread that issues a peer's share of a frame is stopped before anything it uses goes;
//   2. a root, with each rank's device current, waits for EVERY rank's streams, then destroys the communicators, then the peers: no
//      communicator outlives a stream it was used on, no all_slabs is freed under a running all-gather;
//   3. this context's own streams are waited for (not left to the implicit synchronisation of a free).
ycge_ctx::~ycge_ctx()
{
    try {
        stop_worker();
        for (ycge_ctx *p : peers) p->stop_worker();
        for (ycge_ctx *p : peers) p->drain();
        drain();
        if (!nccl_comms.empty()) {
            const RcclApi &R = load_rccl();
            for (void *cm : nccl_comms) if (cm && R.CommDestroy) (void)R.CommDestroy(cm);
            nccl_comms.clear();
        }
        for (ycge_ctx *p : peers) delete p;
        peers.clear();
        (void)hipSetDevice(device);
    }
    catch (...) { }
}

extern "C" {

const char *ycge_last_error(const ycge_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int ycge_device_info(ycge_ctx *c, char *name, size_t name_bytes, int32_t *compute_units)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (name && name_bytes) { std::strncpy(name, c->device_name, name_bytes - 1); name[name_bytes - 1] = 0; }
    if (compute_units) *compute_units = c->compute_units;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
namespace ycge_host {

// ---- device -> host.  The device writes host memory in two places only: page-locked memory (the library's own - hipHostMalloc - or whole
// pages the caller registered, ycge_pin_host_buffer) and the library's own staging buffer below; a PAGEABLE destination is filled by the CPU
// from that staging buffer.  Handing a pageable pointer to hipMemcpy lets the runtime choose how the bytes get there, and for transfers of
// a megabyte and more it page-locks the caller's pages on the fly and lets the copy engine write them: a mapping of process heap whose
// lifetime neither the caller nor the library controls (the allocator trims and regrows the heap, the runtime caches what it pinned).
// Twice in ~25 runs of the GPU suite in round 4 and once in the first full run of round 5 - AFTER the registered arrays of the Python
// mirror had been given pages of their own - a read-back died with "Memory access fault by GPU ... Write access" at a heap address.
// (the WHOLE range [p, p + bytes): a destination that starts inside a page-locked block and runs past its end - a registered sub-range, an
// array sized for an older console - would let the copy engine write pageable heap behind it, the very fault class this exists to exclude.
// The runtime is asked for the allocation the first byte lies in (hipMemGetAddressRange on its device alias: base and size of the block
// hipHostMalloc / hipHostRegister made) and the range must end inside it; a runtime that cannot say is asked about the last byte too, and
// the two ends must be page-locked host memory whose device aliases lie exactly as far apart as the host addresses.  Anything else is
// answered "no": the staging copy is always right.)
bool host_memory_is_page_locked(const void *p, size_t bytes)
{
    auto locked = [](const void *q, hipPointerAttribute_t &a) {
        std::memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }      // (older runtimes: an error for plain heap memory)
        return a.type == hipMemoryTypeHost;
    };
    hipPointerAttribute_t a0, a1;
    if (!locked(p, a0)) return false;
    if (bytes <= 1) return true;
    hipDeviceptr_t base = nullptr;
    size_t block = 0;
    if (a0.devicePointer && hipMemGetAddressRange(&base, &block, (hipDeviceptr_t)a0.devicePointer) == hipSuccess && base && block) {
        const uint8_t *b = (const uint8_t *)base, *d = (const uint8_t *)a0.devicePointer;
        return d >= b && (size_t)(d - b) <= block && bytes <= block - (size_t)(d - b);
    }
    (void)hipGetLastError();
    if (!locked((const uint8_t *)p + (bytes - 1), a1)) return false;
    return a0.devicePointer && a1.devicePointer && (const uint8_t *)a1.devicePointer - (const uint8_t *)a0.devicePointer == (ptrdiff_t)(bytes - 1);
}
// synchronous copy of `bytes` from device memory of the current device to `dst`; nothing of this context may be in flight on other streams
int copy_out(ycge_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return YCGE_OK;
    if (host_memory_is_page_locked(dst, bytes)) { HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return YCGE_OK; }
    const size_t chunk = (size_t)32 << 20;
    HIP_TRY(c, c->out_stage.reserve(bytes < chunk ? bytes : chunk));
    for (size_t off = 0; off < bytes; off += chunk) {
        const size_t n = bytes - off < chunk ? bytes - off : chunk;
        HIP_TRY(c, hipMemcpyAsync(c->out_stage.p, (const uint8_t *)src + off, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::memcpy((uint8_t *)dst + off, c->out_stage.p, n);
    }
    return YCGE_OK;
}

// every stream a frame of this context may still be running on
int quiesce(ycge_ctx *c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    // a pipelined tiled caller may alternate several streams of its own between ycge_trace_tiles and ycge_resolve_gathered; the
    // scene updates rewrite live allocations in place (DevBuf::upload), so wait for the whole device - this is a per-scene-change
    // call, never part of a frame
    HIP_TRY(c, hipDeviceSynchronize());
    c->async_outstanding = false; c->set_read[0] = c->set_read[1] = c->set_read[2] = false;        // (frames in flight included)
    c->post_hist_pending = c->post_busy = c->post_set_pending[0] = c->post_set_pending[1] = c->post_set_pending[2] = false;
    return YCGE_OK;
}

} // namespace ycge_host
extern "C" {
// profiling aid: the progress lines of the persistent in-place A-trous launch (32 words per band: [0] progress, [4..7] begin / end
// timestamps at 100 MHz, [8] passes) of the last frame with a post stage
int ycge_debug_read_post_progress(ycge_ctx *c, uint32_t *dst, size_t n_words)
try {
    if (!c || !dst || !c->post_progress.p || n_words > c->post_progress.n) return YCGE_ERR_INVALID_ARG;
    HIP_TRY(c, hipDeviceSynchronize());
    return copy_out(c, dst, c->post_progress.p, n_words * 4);
}
catch (...) { return ycge_host::abi_catch(c); }

// OBJ meshes from file bytes (ycge_obj.cpp): MeshLoader.FromObj up to the triangles ycge_mesh.triangles takes.  The host parser alone ...
int ycge_obj_parse_host(const uint8_t *text, size_t bytes, float *positions, int32_t *faces, ycge_obj_info *info, char *msg, size_t msg_bytes)
try {
    return obj_parse_host(text, bytes, positions, faces, info, msg, msg_bytes);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ... the parse on the device, held by the context ...
int ycge_obj_parse(ycge_ctx *c, const uint8_t *text, size_t bytes, ycge_obj_info *info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return obj_parse(c, text, bytes, info);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... its positions and faces ...
int ycge_obj_read(ycge_ctx *c, float *positions, int32_t *faces)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return obj_read(c, positions, faces);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... FromObj's tail: normalise, scale / translate, gather, bounds ...
int ycge_obj_triangles(ycge_ctx *c, int32_t normalize, float target_size, float scale, const float translate[3], float *out_triangles, float out_bounds[6])
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return obj_triangles(c, normalize, target_size, scale, translate, out_triangles, out_bounds);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... MeshScenes.TryReadObjBoundsNormalized behind its parse: the host tail alone ...
int ycge_obj_ground_host(const float *positions, int32_t n_positions, const int32_t *faces, int32_t n_triangles, ycge_obj_ground_info *out)
try {
    return obj_ground_host(positions, n_positions, faces, n_triangles, out);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ... the same on the held OBJ, on the device ...
int ycge_obj_ground(ycge_ctx *c, ycge_obj_ground_info *out)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return obj_ground(c, out);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... and AddMeshAutoGround's placed triangles in one call
int ycge_obj_triangles_auto_ground(ycge_ctx *c, float scale, const float target[3], float *out_triangles, float out_bounds[6], ycge_obj_ground_info *out_info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return obj_triangles_auto_ground(c, scale, target, out_triangles, out_bounds, out_info);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_obj_release(ycge_ctx *c)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return obj_release(c);
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hook: who parsed, why, and the last parse's phases (include/ycge_hooks.h)
int ycge_debug_obj_stats(ycge_ctx *c, int64_t *out6)
try {
    return obj_stats(c, out6);
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hooks: who took the auto-ground tail, why, its rounds and time; with YCGE_OBJ_GROUND_PHASES, what each phase cost (include/ycge_hooks.h)
int ycge_debug_obj_ground_stats(ycge_ctx *c, int64_t *out6)
try {
    return obj_ground_stats(c, out6);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_debug_obj_ground_phases(ycge_ctx *c, int64_t *out5)
try {
    return obj_ground_phases(c, out5);
}
catch (...) { return ycge_host::abi_catch(c); }

// a VG01 world file's header (ycge_world_store.cpp: pure host code, no context and no device) ...
int ycge_world_file_info(const uint8_t *bytes, size_t n_bytes, int32_t dims_out[3], size_t *payload_offset_out, char *msg, size_t msg_bytes)
try {
    return world_file_info(bytes, n_bytes, dims_out, payload_offset_out, msg, msg_bytes);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// ... its payload made resident on every device of the context, what the context holds of it, given back ...
int ycge_world_store_load(ycge_ctx *c, const int32_t *cells, int32_t nx, int32_t ny, int32_t nz, int32_t chunk_size)
try {
    return world_store_load(c, cells, nx, ny, nz, chunk_size);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_world_store_info(ycge_ctx *c, int32_t dims_out[3], int32_t *chunk_size_out, uint8_t *occupied_out, size_t capacity)
try {
    return world_store_info(c, dims_out, chunk_size_out, occupied_out, capacity);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_world_store_release(ycge_ctx *c)
try {
    return world_store_release(c);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... and its chunks attached by key (AttachChunkFromPreloaded)
int ycge_scene_attach_world_chunks(ycge_ctx *c, const int32_t *keys, int32_t n, const ycge_grid *proto, int32_t *out_grid_index)
try {
    return world_store_attach(c, keys, n, proto, out_grid_index);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... the store made by the generator on the device instead of loaded, and its payload read back in x-planes (a VG01 file, slab by slab)
int ycge_world_store_generate(ycge_ctx *c, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t form)
try {
    return world_store_generate(c, world, chunks_x, chunks_z, origin_bx, origin_bz, form);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_world_store_read(ycge_ctx *c, int32_t x0, int32_t planes, int32_t *cells_out)
try {
    return world_store_read(c, x0, planes, cells_out);
}
catch (...) { return ycge_host::abi_catch(c); }

// voxel edits: cells of resident grids (ycge_grid_edit.cpp) and of the world store (ycge_world_store.cpp) changed where they lie
int ycge_scene_edit_voxels(ycge_ctx *c, const ycge_voxel_edit *ops, int32_t n, uint32_t *out_info)
try {
    return scene_edit_voxels(c, ops, n, out_info);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_world_store_edit(ycge_ctx *c, const ycge_voxel_edit *ops, int32_t n)
try {
    return world_store_edit(c, ops, n);
}
catch (...) { return ycge_host::abi_catch(c); }

// the pool of materialised chunks that lets a fields store take edits (ycge_world_store.cpp)
int ycge_world_store_reserve_edits(ycge_ctx *c, int32_t max_chunks)
try {
    return world_store_reserve_edits(c, max_chunks);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_world_store_edit_slots(ycge_ctx *c, int32_t *capacity_out, int32_t *used_out)
try {
    return world_store_edit_slots(c, capacity_out, used_out);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_world_store_revert_chunks(ycge_ctx *c, const int32_t *keys, int32_t n)
try {
    return world_store_revert_chunks(c, keys, n);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_debug_world_store_generate_stats(ycge_ctx *c, int64_t *out9)
try {
    return world_store_generate_stats(c, out9);
}
catch (...) { return ycge_host::abi_catch(c); }

// test / profiling hooks: one chunk's raw cells as the slice writes them (no attach); the store's size, the last load's and attach's split (include/ycge_hooks.h)
int ycge_debug_world_store_chunk(ycge_ctx *c, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t dims_out[3])
try {
    return world_store_chunk(c, cx, cy, cz, cells_out, dims_out);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_debug_world_store_stats(ycge_ctx *c, int64_t *out8)
try {
    return world_store_stats(c, out8);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_resize(ycge_ctx *c, int32_t fbw, int32_t fbh, int32_t ss)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    const int rc = on_root_then_peers(c, [&](ycge_ctx *x) { const int qrc = quiesce(x); return qrc != YCGE_OK ? qrc : set_geometry(x, fbw, fbh, ss); });
    (void)hipSetDevice(c->device);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_set_camera(ycge_ctx *c, const float pos[3], float yaw, float pitch, float fov_deg)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!pos) return c->fail(YCGE_ERR_INVALID_ARG, "null position");
    std::lock_guard<std::mutex> g(c->cam_lock);
    c->cam_pos[0] = pos[0]; c->cam_pos[1] = pos[1]; c->cam_pos[2] = pos[2];
    c->yaw = yaw; c->pitch = pitch; c->fov_deg = fov_deg;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_set_frame_counter(ycge_ctx *c, int64_t fc)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (fc < 0 || fc == INT64_MAX) return c->fail(YCGE_ERR_INVALID_ARG, "frame counter must be in [0, 2^63 - 2] (the reference's counter starts at 0 and only grows, RaytraceRenderer.cs:24,175)");
    c->frame_counter = fc;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// profiling builds: the 6 sums of the cooperative walk's statistics (ycge_coop.hip.h, -DYCGE_DBG_COOPSTAT), cumulative
int ycge_debug_read_coop_stats(ycge_ctx *c, uint64_t out[16])
try {
    if (!c || !out || !c->dbg_counters.p) return YCGE_ERR_INVALID_ARG;
    std::vector<unsigned long long> v(16 + 16 * 256);
    HIP_TRY(c, hipDeviceSynchronize());
    { const int rc2 = copy_out(c, v.data(), c->dbg_counters.p, v.size() * sizeof(unsigned long long)); if (rc2 != YCGE_OK) return rc2; }
    for (int k = 0; k < 16; k++) { out[k] = 0; for (int i = 0; i < 256; i++) out[k] += v[16 + 8 * 256 * (k >> 3) + 8 * i + (k & 7)]; }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// profiling builds (-DYCGE_DBG_BATCHSTAT, mesh_walk): 8 banks of 8 sums, cumulative; banks 2-4 every batch by kind (occlusion / closest hit / mixed),
// 5-7 the batches of >= 48 iterations
int ycge_debug_read_batch_stats(ycge_ctx *c, uint64_t out[64])
try {
    if (!c || !out || !c->dbg_counters.p) return YCGE_ERR_INVALID_ARG;
    std::vector<unsigned long long> v(16 + 64 * 256);
    HIP_TRY(c, hipDeviceSynchronize());
    { const int rc2 = copy_out(c, v.data(), c->dbg_counters.p, v.size() * sizeof(unsigned long long)); if (rc2 != YCGE_OK) return rc2; }
    for (int k = 0; k < 64; k++) { out[k] = 0; for (int i = 0; i < 256; i++) out[k] += v[16 + 8 * 256 * (k >> 3) + 8 * i + (k & 7)]; }
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// Page-locked host memory for the SDR frame.  hipHostRegister works on whole pages: two registered heap arrays that share a boundary page
// lose it when ONE of them is unregistered, and the other's next read-back is a device write to an unmapped host page ("Memory access fault
// by GPU" at a heap address, round 4).  So the library refuses a range that is not whole pages of its own - the caller proves it owns the
// pages by handing over page-aligned memory - and offers memory that is (ycge_alloc_host_buffer: hipHostMalloc).
size_t ycge_host_page_size(void)
try {
    const long p = sysconf(_SC_PAGESIZE);
    return p > 0 ? (size_t)p : (size_t)4096;
}
catch (...) { (void)ycge_host::abi_catch(nullptr); return 0; }
int ycge_pin_host_buffer(void *buffer, size_t bytes)
try {
    const size_t page = ycge_host_page_size();
    if (!buffer || bytes == 0 || ((uintptr_t)buffer % page) != 0 || (bytes % page) != 0) return YCGE_ERR_INVALID_ARG;
    if (hipHostRegister(buffer, bytes, hipHostRegisterDefault) == hipSuccess) return YCGE_OK;
    (void)hipGetLastError();
    return YCGE_ERR_DEVICE;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
int ycge_unpin_host_buffer(void *buffer)
try {
    if (!buffer || ((uintptr_t)buffer % ycge_host_page_size()) != 0) return YCGE_ERR_INVALID_ARG;
    if (hipHostUnregister(buffer) == hipSuccess) return YCGE_OK;
    (void)hipGetLastError();
    return YCGE_ERR_DEVICE;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
int ycge_alloc_host_buffer(size_t bytes, void **out)
try {
    if (!out) return YCGE_ERR_INVALID_ARG;
    *out = nullptr;
    if (bytes == 0) return YCGE_ERR_INVALID_ARG;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return YCGE_ERR_OUT_OF_MEMORY; }
    std::memset(p, 0, bytes);
    *out = p;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }
int ycge_free_host_buffer(void *buffer)
try {
    if (!buffer) return YCGE_OK;
    if (hipHostFree(buffer) == hipSuccess) return YCGE_OK;
    (void)hipGetLastError();
    return YCGE_ERR_INVALID_ARG;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_device_count(void)
try {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : -1;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_read_timed_steps(ycge_ctx *c, uint64_t *lane_steps)
try {
    if (!c || !lane_steps) return YCGE_ERR_INVALID_ARG;
    unsigned long long total = 0;
    for (ycge_ctx *d : contexts_of(c)) {
        std::vector<unsigned long long> v(YCGE_COUNTER_WORDS);
        if (hipSetDevice(d->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            copy_out(d, v.data(), d->counters.p, v.size() * sizeof(unsigned long long)) != YCGE_OK) { (void)hipSetDevice(c->device); return c->fail(YCGE_ERR_DEVICE, "timed-step read-back failed on device %d", d->device); }
        for (size_t i = 8; i < v.size(); i += 8) total += v[i];
    }
    (void)hipSetDevice(c->device);
    *lane_steps = total;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_tile_slab_bytes(const ycge_ctx *c, size_t *bytes)
try {
    if (!c || !bytes) return YCGE_ERR_INVALID_ARG;
    *bytes = (size_t)c->tiles_per_rank_padded * 256 * slab_floats(c) * sizeof(float);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// sizeof of each ABI struct, for the ctypes mirror check
size_t ycge_abi_sizeof(int32_t which)
try {
    switch (which) {
    case 0: return sizeof(ycge_vec3); case 1: return sizeof(ycge_material); case 2: return sizeof(ycge_prim); case 3: return sizeof(ycge_mesh);
    case 4: return sizeof(ycge_voxel_lookup); case 5: return sizeof(ycge_grid); case 6: return sizeof(ycge_light); case 7: return sizeof(ycge_scene);
    case 8: return sizeof(ycge_config); case 9: return sizeof(ycge_frame_stats); case 10: return sizeof(ycge_flight_info);
    case 11: return sizeof(ycge_world); case 12: return sizeof(ycge_ansi_async); case 13: return sizeof(ycge_ansi_async_result);
    }
    return 0;
}
catch (...) { (void)ycge_host::abi_catch(nullptr); return 0; }

// tests: what copy_out / run_post / ycge_render_frame_async_sdr decide about a destination (1: the device may write [p, p + bytes) directly)
int ycge_debug_is_page_locked(const void *p, size_t bytes)
try {
    return (p && host_memory_is_page_locked(p, bytes)) ? 1 : 0;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// tests (tests/test_host_cpu.py, no GPU needed): an exception of the given kind raised INSIDE an exported body - what comes back is the
// barrier's answer (abi_catch): 1 std::bad_alloc, 2 std::runtime_error, 3 something that is no std::exception, 4 std::length_error out of a
// vector, 5 std::system_error as a failing std::thread constructor raises it; 0 nothing
int ycge_debug_throw(ycge_ctx *c, int32_t kind)
try {
    if (kind == 1) throw std::bad_alloc();
    if (kind == 2) throw std::runtime_error("requested by ycge_debug_throw");
    if (kind == 3) throw 42;
    if (kind == 4) { std::vector<uint64_t> v; v.resize(v.max_size() + (size_t)kind); }
    if (kind == 5) throw std::system_error(std::make_error_code(std::errc::resource_unavailable_try_again), "thread");
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// tests: what the process holds through the owners of ycge_own.h right now - {device allocations, device bytes, events, streams, page-locked
// allocations, page-locked bytes}.  Needs no context and no device.
int ycge_debug_live_resources(int64_t out[6])
try {
    if (!out) return YCGE_ERR_INVALID_ARG;
    for (int k = 0; k < LIVE_KINDS; k++) out[k] = g_live[k].load(std::memory_order_relaxed);
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

#if YCGE_FAULT_INJECTION
// lib/var_faultinject.so only (tests/test_gpu_abi_barrier.py): the n-th allocation from now fails.  The replaced operators serve this
// library's own code (every std::vector, std::string and `new` of the host side is compiled into it; -Bsymbolic binds them here).
int ycge_debug_fail_allocation(int64_t nth)
{
    const long long left = g_fail_alloc_countdown.exchange((long long)nth);
    return left < 0 ? -1 : (int)(left > 0x7fffffff ? 0x7fffffff : left);
}
#endif

} // extern "C"
#if YCGE_FAULT_INJECTION && !defined(__HIP_DEVICE_COMPILE__)
// (the variant is linked -Wl,-Bsymbolic: the library's own references bind to these definitions, whatever else the process has loaded)
static void *fi_alloc(std::size_t n)
{
    if (g_fail_alloc_countdown.load(std::memory_order_relaxed) >= 0 && g_fail_alloc_countdown.fetch_sub(1) == 0) throw std::bad_alloc();
    void *p = std::malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void *operator new(std::size_t n) { return fi_alloc(n); }
void *operator new[](std::size_t n) { return fi_alloc(n); }
void operator delete(void *p) noexcept { std::free(p); }
void operator delete[](void *p) noexcept { std::free(p); }
void operator delete(void *p, std::size_t) noexcept { std::free(p); }
void operator delete[](void *p, std::size_t) noexcept { std::free(p); }
#endif
