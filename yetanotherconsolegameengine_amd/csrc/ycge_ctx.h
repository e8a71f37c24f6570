// ycge_ctx.h - the context of the library (struct ycge_ctx), the launch entry points of the kernel files, and what the host translation
// units share (internal: the C-ABI is include/ycge.h).
//   ycge_host.cpp      context (creation, teardown order), geometry, copy_out / quiesce, the exception barrier, host buffers, general hooks
//   ycge_scene.cpp     scene flattening and upload as named steps, scene updates, the object installs
//   ycge_mesh_bvh.cpp  mesh trees (device builder or host builder) and the mesh arena (device emit or host emit), their hooks
//   ycge_frame.cpp     frame orchestration (TryFlipAndBlit steps 1-5 and 9), frames in flight, the slab form of the tiled frame
//   ycge_post_host.cpp the post stage (steps 6-8) and its schedules
//   ycge_resident.cpp  the tile-resident multi-GPU form, its batched launches and emulation loop; read-backs (ycge_read_buffer / _accel)
//   ycge_query.cpp, ycge_chexel.cpp, ycge_ansi.cpp, ycge_grid_encode.cpp, ycge_worldgen_scene.cpp   scene queries, chexel colours, the ANSI stream, streamed grids, generated chunks
//   ycge_grid_edit.cpp     voxel edits of resident grids (ycge_scene_edit_voxels): pair -> code, the brick work list, the records that follow
//   ycge_world_store.cpp   a VG01 world resident on the device - loaded, or generated there - its chunks attached by key, its planes read back
//   ycge_accel.cpp     the bit-faithful BVH builders
// Every GPU resource is held through an owner of ycge_own.h: members free themselves, ycge_ctx::~ycge_ctx orders only what has an order.
// All device work is in the .hip files; there is no CPU implementation of any per-pixel stage.
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <string>
#include <vector>
#include <functional>

#include "../../include/ycge.h"
#include "ycge_accel.h"
#include "ycge_ansi_layers.h"
#include "ycge_device.h"
#include "ycge_math.h"
#include "ycge_mesh_pool.h"
#include "ycge_own.h"
#include "ycge_world_store.h"
#include "ycge_worldgen.h"

extern "C" {
size_t ycge_wf_sizes(int which);
int ycge_launch_trace(const ycge::SceneDev *S, const ycge::FrameParams *P, const ycge::TraceOut *O, int count, int flat,
                      hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
int ycge_launch_wavefront(const ycge::SceneDev *S, const ycge::FrameParams *P, const ycge::TraceOut *O, void *const bufs[7], int rounds,
                          int has_grid, int flat, int count, int persistent_waves, hipStream_t stream, hipStream_t side, hipEvent_t ev_fork, hipEvent_t ev_join,
                          const ycge::TraceOut *O_side);
int ycge_launch_trace_batch(const ycge::SceneDev *S, const ycge::FrameParams *P, const ycge::TraceOut *O, int n, int count, int flat, hipStream_t stream);
int ycge_launch_scene_walk(const void *nodes, int n_inner, const uint32_t *leaf_prims, const void *prims, void *walk, hipStream_t stream);
int ycge_launch_order_blocks(uint32_t *cost, uint32_t n, uint32_t policy, uint32_t split_top, uint32_t next_slot, uint32_t skip_mask, uint32_t *order_ws,
                             uint32_t *order, hipStream_t stream, int small_groups = 0, uint32_t n_frames = 0, uint32_t *snap = nullptr);
int ycge_launch_taa_tiles(const ycge::TaaParams *T, const ycge::FrameParams *P, const float *current, const float *normal, const float *depth, const uint8_t *sky,
                          float *hist, const ycge::TaaGuides *prev_in, const ycge::TaaGuidesOut *prev_out /* null: no guide store */, float *slab, hipStream_t stream);
int ycge_launch_resolve_tiles(const ycge::TaaParams *T, const ycge::FrameParams *P, const float *current, const float *normal, const float *depth, const uint8_t *sky,
                              const void *records, const uint32_t *halo_index, float *hist, const ycge::TaaGuides *prev_in, const ycge::TaaGuidesOut *prev_out /* null: no guide store */, float *slab, hipStream_t stream);
int ycge_launch_halo(int scatter, float *hdr, uint8_t *sky, const uint32_t *px, uint32_t n, void *records, hipStream_t stream);
int ycge_launch_pack_history(const ycge::FrameParams *P, const float *hist, float *slab, hipStream_t stream);
int ycge_launch_unpack_history(const float *all_slabs, size_t slab_floats_per_rank, int hiW, int hiH, int tiles_x, int n_tiles, int world_size, float *hist, hipStream_t stream);
int ycge_launch_taa(const ycge::TaaParams *T, const float *current, const float *normal, const float *depth, const uint8_t *sky,
                    float *hist, const ycge::TaaGuides *prev_in, const ycge::TaaGuidesOut *prev_out, hipStream_t stream, int small_groups = 0, hipEvent_t stop = nullptr);
size_t ycge_post_state_bytes(void);
int ycge_atrous_persist_resident(int groups_per_pass, int split, int profile);
void ycge_atrous_duo_pad_lds(int bytes);
int ycge_launch_unit_normals(const float *normal, float *unit, size_t n, hipStream_t stream);
int ycge_launch_atrous(int w, int h, int step, const float phi[4], const float *cur, float *dst, const float *albedo, const float *unit_n,
                       const float *depth, const uint8_t *sky, hipStream_t stream);
int ycge_launch_atrous_static(int w, int h, int step, const float phi[4], const float *albedo, const float *unit_n, const float *depth,
                              const uint8_t *sky, float *statw, hipStream_t stream);
int ycge_launch_atrous_inplace(int w, int h, int step, const float phi[4], float *buf, const float *albedo, const float *unit_n,
                               const float *depth, const uint8_t *sky, float *statw, const uint32_t *d_pixels, const uint32_t *d_offsets,
                               int n_levels, int n_bands, int K, int groups_per_pass, int rows_per_band, unsigned window_width, hipStream_t stream);
int ycge_launch_atrous_persist(int w, int h, int step, const float phi[4], float *buf, const uint8_t *sky, float *statw, const uint32_t *d_pixels,
                               const uint32_t *d_offsets, const uint32_t *d_pass_level, const int32_t *d_band_desc, int n_levels, int n_bands, int groups_per_pass, int rows_per_band, unsigned window_width,
                               uint32_t *progress, uint32_t epoch, int xcd_local, int profile, uint32_t ticket_base, hipStream_t stream);
size_t ycge_exposure_scratch_bytes(int w, int h, int step);
size_t ycge_bvh_build_scratch_bytes(int n);
int ycge_launch_scene_bvh_build(const float *items, int n, void *scratch, void *ref_out, void *gnodes_out, uint32_t *leaf_out, void *result,
                                int active_waves, hipStream_t stream);
size_t ycge_mesh_bvh_sizes(int which);
int ycge_launch_mesh_items(const float *tris9, int n, float *items, uint32_t *hdr, hipStream_t stream);
int ycge_launch_mesh_init(int n, int wide, uint32_t *ord, int32_t *node_of, void *top, int32_t *level0, int32_t *jobs, uint32_t *hdr, hipStream_t stream);
int ycge_launch_mesh_wide_level(const float *items, int n, int n_cur, int wide_min, int next_slot, uint32_t *ord, uint32_t *ord2, int32_t *node_of, const int32_t *level,
                                int32_t *level_next, int32_t *jobs, void *top, int top_cap, void *acc, uint8_t *flag, uint32_t *lpref, uint32_t *blk, uint32_t *blk_excl,
                                uint32_t *back_l, uint32_t *hdr, hipStream_t stream);
int ycge_launch_mesh_subtrees(const float *items, int n, const uint32_t *ord, float *items_pos, const int32_t *jobs, int n_jobs, void *top, void *sub_nodes,
                              uint32_t *leaf_out, uint32_t *hdr, hipStream_t stream);
int ycge_launch_mesh_assemble(void *top, int n_top, int n_levels, const int32_t *jobs, int n_jobs, const void *sub_nodes, void *nodes_out, uint32_t *hdr, hipStream_t stream);
uint32_t ycge_launch_mesh_emit_tiles(uint32_t n_nodes);
int ycge_launch_mesh_emit_layout(const void *nodes, uint32_t n_nodes, uint32_t mesh, uint32_t *tiles, uint32_t *refs, uint32_t *hdr, hipStream_t stream);
int ycge_launch_mesh_emit_records(const void *nodes, uint32_t n_nodes, uint32_t n_tris, uint32_t mesh, const uint32_t *refs, const uint32_t *leaf, const float *tris9,
                                  const int32_t *tri_material, int32_t material, int32_t n_materials, uint8_t *arena, uint32_t arena_units, uint32_t *hdr, hipStream_t stream);
int ycge_launch_mesh_emit_treelets(const uint32_t *refs, uint32_t n_nodes, uint8_t *arena, uint32_t tl_offset, hipStream_t stream);
int ycge_launch_exposure(const float *hdr, const uint8_t *sky, int w, int h, int step, float *terms, void *state, const float consts[5],
                         void *scratch, int serial, hipStream_t stream);
int ycge_launch_exposure_sums(const float *terms, int n, void *state, const float consts[5], void *scratch, int serial, hipStream_t stream);
int ycge_launch_tonemap(const float *hdr, int hiW, int fbW, int fbH, int ss, float gamma, float saturation, float vibrance, const void *state,
                        float *out, hipStream_t stream);
int ycge_launch_pack_slab(const ycge::FrameParams *P, const float *hdr, const float *albedo, const float *normal, const float *depth,
                          const uint8_t *sky, float *slab, int slab_floats, hipStream_t stream);
int ycge_launch_push_tiles(const ycge::FrameParams *P, const ycge::PushPlanes *planes, hipStream_t stream);
int ycge_launch_unpermute(const float *all_slabs, size_t slab_floats_per_rank, int hiW, int hiH, int tiles_x, int n_tiles, int world_size,
                          int slab_floats, float *hdr, float *albedo, float *normal, float *depth, uint8_t *sky, hipStream_t stream);
uint32_t ycge_launch_query_lanes(int has_grid, int occluded, int compute_units);
int ycge_launch_chexels(const float *sdr, int fbW, int fbH, const uint8_t *tables, uint8_t *c16, uint8_t *ansi, uint8_t *rgba, int compute_units, hipStream_t stream);
int ycge_launch_tonemap_quadrants(const float *hdr, int hiW, int fbW, int fbH, int ss, float gamma, float saturation, float vibrance, const void *state,
                                  float *out, hipStream_t stream);
int ycge_launch_quadrant_fit(const float *quad, int fbW, int fbH, const uint8_t *tables, int min_contrast, uint16_t *glyphs, uint8_t *rgba, int compute_units,
                             hipStream_t stream);
int ycge_launch_sixel_pixels(const float *hdr, int W, int H, float gamma, float saturation, float vibrance, const void *state, const uint8_t *tables, int dither,
                             uint8_t *rgba, uint8_t *index, int compute_units, hipStream_t stream);
int ycge_launch_sixel_encode_palette(const uint8_t *index, int W, int H, uint32_t *last1, uint32_t *lines, uint32_t *line_bytes, uint32_t max_lines, uint32_t *meta,
                                     const uint8_t *prefix, uint32_t prefix_bytes, const uint8_t *defs, const uint32_t *defs_bytes, uint8_t *out, uint32_t cap,
                                     unsigned long long *res, int compute_units, hipStream_t stream);
int ycge_launch_sixel_palette(const uint8_t *rgba, int W, int H, int build, uint32_t *hist, uint8_t *block, uint8_t *index, int compute_units, hipStream_t stream);
int ycge_launch_sixel_encode(const uint8_t *index, int W, int H, uint32_t *last1, uint32_t *lines, uint32_t *line_bytes, uint32_t max_lines, uint32_t *meta,
                             const uint8_t *header, uint32_t header_bytes, uint8_t *out, uint32_t cap, unsigned long long *res, int compute_units, hipStream_t stream,
                             const uint8_t *prev = nullptr, uint32_t *span = nullptr);
uint32_t ycge_launch_ansi_tiles(uint32_t cells);
int ycge_launch_ansi_indexed(const ycge_ansi::StreamJob *job, hipStream_t stream);
int ycge_launch_ansi_rgb(const ycge_ansi::StreamJob *job, hipStream_t stream);
int ycge_launch_ansi_deliver(const uint8_t *src, const unsigned long long *res, unsigned long long capacity, int full, uint8_t *dst, void *record, uint32_t *sticky,
                             int groups, hipStream_t stream);
int ycge_launch_video_blit(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, float *sdr, hipStream_t stream);
int ycge_launch_video_blit_quadrants(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, float *sdr, float *quad_sdr,
                                     hipStream_t stream);
int ycge_launch_video_pixels(const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const uint8_t *tables, const uint8_t *srgb_tables, int dither,
                             uint8_t *rgba, uint8_t *index, hipStream_t stream);
size_t ycge_launch_obj_sizes(int which);
int ycge_launch_obj_count_lines(const uint8_t *text, uint32_t n, uint32_t first, uint32_t *tiles, void *header, hipStream_t stream);
int ycge_launch_obj_classify(const uint8_t *text, uint32_t n, uint32_t first, const uint32_t *tiles, uint32_t *line_start, uint32_t n_lines, uint32_t *add,
                             uint32_t *block_pos, uint32_t *block_tri, void *header, hipStream_t stream);
int ycge_launch_obj_parse(const uint8_t *text, uint32_t n, const uint32_t *line_start, uint32_t n_lines, const uint32_t *add, const uint32_t *block_pos,
                          const uint32_t *block_tri, float *positions, int32_t *faces, uint32_t n_positions, uint32_t n_triangles, void *header, hipStream_t stream);
int ycge_launch_obj_used_bounds(const float *positions, const int32_t *faces, uint32_t n_positions, uint32_t n_triangles, uint8_t *used, void *header, hipStream_t stream);
int ycge_launch_obj_triangles(const float *positions, const int32_t *faces, uint32_t n_triangles, int normalize, const float c[3], float s, int transform,
                              float scale, const float t[3], float *out, void *header, hipStream_t stream);
size_t ycge_launch_obj_ground_sizes(int which);
int ycge_launch_obj_ground_round(const int32_t *faces, uint32_t n_triangles, uint32_t n_positions, uint32_t *parent, int first, void *header, hipStream_t stream);
int ycge_launch_obj_ground_select(const int32_t *faces, uint32_t n_triangles, uint32_t n_positions, const uint32_t *parent, uint32_t *count, uint32_t *first, void *header,
                                  hipStream_t stream);
int ycge_launch_obj_ground_terms(const float *positions, const int32_t *faces, uint32_t n_triangles, uint32_t n_positions, const uint32_t *parent, float *terms, uint32_t padded,
                                 uint8_t *used, void *header, hipStream_t stream);
int ycge_launch_obj_ground_sum(const float *terms, uint32_t padded, void *header, hipStream_t stream);
int ycge_launch_obj_ground_bounds(const float *positions, uint32_t n_positions, const uint8_t *used, void *header, hipStream_t stream);
int ycge_launch_grid_encode(const void *descs, int n_grids, void *results, uint32_t n_workgroups, hipStream_t stream);
int ycge_launch_grid_edit(uint8_t *arena, const void *records, uint32_t n_records, const void *ops, uint32_t *counters, hipStream_t stream);
int ycge_launch_grid_solid(const uint8_t *arena, const void *descs, int n_grids, void *results, uint32_t n_workgroups, hipStream_t stream);
int ycge_launch_query(const ycge::SceneDev *S, const float *rays, uint32_t n, float *hits, int32_t *ids, uint8_t *occluded, uint32_t *first_bad,
                      void *spill, uint32_t lanes, int has_grid, hipStream_t stream);
// the camera tick (k_camera_tick, ycge_camera.hip): one wavefront; in / out: ycge_cam::TickIn / TickOut (ycge_camera_physics.h), spill: 64 columns
int ycge_launch_camera_tick(const ycge::SceneDev *S, const void *in, void *out, void *spill, int has_grid, hipStream_t stream);
// many bodies a tick (k_bodies_tick, ycge_camera.hip): n workgroups of one wavefront; header / in / out: ycge_cam::BodiesHeader, n BodyIn, n TickOut;
// moves: every body's, one array; spill: max(1, spill levels) x 64 * n columns
int ycge_launch_bodies_tick(const ycge::SceneDev *S, const void *header, const void *in, const void *moves, void *out, void *spill, int n, int has_grid,
                            hipStream_t stream);
}

using namespace ycge;

// ycge_scene_upload assembles the arena on the device when a tree built there has this many triangles: the smallest measured count from which
// on that upload is no slower than the same upload with the host's emit (4 000: 1.53 against 1.44 ms; 16 000: 2.37 against 2.82; config 4:
// 11.7 against 198 - profiles/mesh_build_rate.json).  Below it the emit's own allocations and two read-backs outweigh the host's loops.
#define YCGE_MESH_EMIT_DEV_MIN_TRIS_DEFAULT 16000

// ycge_obj_parse hands a file of fewer bytes than this to the host parser: the crossover between ycge_obj_parse_host and the device path
// (profiles/obj_rate.py) is NOT YET MEASURED, so every file goes to the device.
#define YCGE_OBJ_DEVICE_MIN_DEFAULT 0

// ycge_obj_ground hands an OBJ of fewer triangles than this to the host tail (ycge_obj_ground_host): the measured crossover between
// ycge_obj_read + the host tail and the kernels of ycge_obj_ground.hip (profiles/obj_ground_rate.json: at 131 081 triangles 0.95 ms against
// 1.05, at 871 209 3.4 against 9.3; at 16 009 the host side wins, 0.16 against 0.24: the tail's launches and two read-backs cost 0.14 ms
// before any work is done).
#define YCGE_OBJ_GROUND_DEVICE_MIN_DEFAULT 131081

namespace ycge_host {

inline std::string g_create_error;          // (one per library: C++17 inline variable)
// THE EXCEPTION BARRIER of the C-ABI (round 6): every exported function's body is a function-try-block whose handler ends here, so that no
// C++ exception - std::bad_alloc from a vector that flattens an 871 200-triangle mesh, std::system_error from a thread constructor - unwinds
// into the P/Invoke frame of the CLR host ("no exceptions/longjmp across the ABI").  Called INSIDE a catch (...) handler:
// rethrows to classify.  std::bad_alloc -> YCGE_ERR_OUT_OF_MEMORY, anything else -> YCGE_ERR_INTERNAL; the text goes to ycge_last_error.
int abi_catch(const ycge_ctx *c) noexcept;

// Experiment knobs (none changes a pixel): read ONCE, when the context is created.
struct Knobs {
    int path_policy = 0;             // YCGE_PATH: 0 auto, 1 wavefront, 2 single launch
    bool xcd_strips = false, generic_walk = false, no_lpt = false, no_refill = false;
    int wave_prof_stage = -1;        // YCGE_WAVE_PROF: -1 off, 0 primary, 1 extend, 2 mega
    bool split_set = false; uint32_t split_policy = 0;
    int split_top_lg = 2;                        // YCGE_SPLIT_TOP_LG: log2 of the parts such a block goes in (2 = 4 parts of 16 pixels)
    bool split_top_set = false;                  // YCGE_SPLIT_TOP / YCGE_SPLIT_TOP_LG given: they decide; else schedule_policy picks by the frame's block count
    int split_top = YCGE_SPLIT_TOP_DEFAULT;     // YCGE_SPLIT_TOP: this many blocks at the head of the schedule go in 4 parts of 16 pixels (0 = none)
    int pw_per_cu = 32;
    int post_band_rows = YCGE_POST_BAND_ROWS_DEFAULT, post_k = YCGE_POST_K_DEFAULT, post_groups = YCGE_POST_GROUPS_DEFAULT;
    bool traced_packet = false;      // YCGE_TRACED_PACKET=1: the synchronous frame records an event between the trace and TAA for the side stream's schedule, as before (A/B)
    bool taa_copy_guides = false;    // YCGE_TAA_COPY_GUIDES=1: the synchronous single-device frame copies TAA's guide planes as every other form does (A/B; same pixels)
    bool split_resolve = false;      // YCGE_RES_SPLIT_RESOLVE=1: the tile-resident resolve as round 5's two launches (k_scatter_halo, k_taa_tiles) instead of k_resolve_tiles (A/B)
    int post_mode = 0;               // YCGE_POST_MODE: in-place A-trous: 0 = one persistent launch, level-granular hand-over (k_atrous_stream), 2 = a launch per level group, 3 = as 0 with bands in block order
    bool post_no_split = false;      // YCGE_POST_NO_SPLIT: whole bands in the persistent in-place A-trous (no row-parity half-bands)
    int post_probe_band = -1;        // YCGE_POST_PROBE_BAND: this band and the next record a per-pass timeline (profiles/post_bands.py)
    int post_assume_resident = 0;    // YCGE_POST_ASSUME_RESIDENT (tests): take this for the runtime's answer - more bands than fit, to exercise the order-of-arrival numbering
    bool post_dbg_free = false;      // YCGE_POST_DBG_FREE (timing experiment, WRONG pixels): no band of the persistent in-place A-trous waits for the band above
    bool flight_small_groups = true; // YCGE_FLIGHT_SMALL_GROUPS: TAA and schedule kernels of the frames in flight in small workgroups (they find room beside a running trace)
    int flight_priority = 1;         // YCGE_FLIGHT_PRIORITY: the second stream's priority: 1 highest, 0 normal, -1 lowest
    bool flight_post_pair = true;    // YCGE_FLIGHT_POST_PAIR: the post stages of consecutive frames in flight side by side (second set of denoise buffers)
    bool flight_placed_gate = true;  // YCGE_FLIGHT_PLACED_GATE: a frame in flight traces once the trace before it has placed its last workgroup (a value that kernel stores)
    bool flight_post_gate = true;    // YCGE_FLIGHT_POST_GATE: a frame in flight traces only once the post stage before it has passed its first iteration
    bool flight_overlap = true;      // YCGE_FLIGHT_OVERLAP: frames in flight alternate between two trace streams (two traces may overlap)
    bool flight_no_begin = false;      // experiments on ycge_render_frame_async: second stream at normal priority; no begin-of-trace timing event
    int post_pad_lds = 0;            // YCGE_POST_PAD_LDS (experiment): bytes of unused LDS per band workgroup of the two-set form - fewer of them on a CU
    int post_resident_per_cu = 3;    // YCGE_POST_RESIDENT: band workgroups of the persistent in-place A-trous a CU may hold (3 fit: 576 threads, 46 KB of LDS each)
    bool post_hash = false;          // YCGE_POST_HASH_FORM=1: the hash form of k_atrous_band even where the window fits
    int bvh_waves = 16;              // YCGE_BVH_WAVES: wavefronts of k_scene_bvh_build that take nodes (tests: the order nodes are split in must not matter)
    bool scene_bvh_host = false;     // YCGE_SCENE_BVH_HOST: ycge_scene_update_objects builds the scene BVH on the host, not on the device
    int scene_bvh_device_min = YCGE_BVH_DEV_MIN_ITEMS_DEFAULT;   // YCGE_SCENE_BVH_DEVICE_MIN: fewer objects than this are built on the host (measured crossover, profiles/r02/f2_update_objects_timing.txt)
    bool mesh_bvh_host = false;      // YCGE_MESH_BVH_HOST: ycge_scene_upload builds every mesh BVH on the host
    int mesh_bvh_device_min = YCGE_MESH_BVH_DEV_MIN_TRIS_DEFAULT;   // YCGE_MESH_BVH_DEVICE_MIN: meshes of fewer triangles are built on the host (measured crossover of the whole upload, profiles/mesh_build_rate.json)
    int mesh_bvh_wide_min = YCGE_BVH_DEV_MAX_ITEMS;   // YCGE_MESH_BVH_WIDE_MIN: nodes of more items take the several-workgroup path of ycge_mesh_bvh_build.hip (9 .. the one-workgroup capacity; tests: many wide levels on small meshes)
    int res_sched_every = 0;         // YCGE_RES_SCHED_EVERY: the tile-resident ring builds a new schedule behind every n-th frame (0 = the ring's depth)
    int bfs_rays = 0;                // YCGE_BFS=<n>: a wavefront's occlusion queries against a mesh go breadth-first from one shared work list when at most n of its lanes ask (mesh_anyhit_bfs; 0 = never, 64 = always)
    bool no_flight_stage_overlap = false;   // YCGE_NO_FLIGHT_STAGE_OVERLAP: frames in flight of the stage pipeline (voxel worlds) one trace at a time (A/B)
    bool no_lights_beside = false;   // YCGE_NO_LIGHTS_BESIDE: the stage pipeline strictly in sequence (A/B of the light loop beside the next round's trace)
    bool lpt_always = false;         // YCGE_LPT_ALWAYS: the longest-first schedule also for frames whose blocks are all resident at once
    int persist_min_tiles = -1;      // YCGE_PERSIST_MIN_TILES: frames of fewer tiles take k_wf_extend instead of the persistent extend stage (-1: a quarter of the persistent wavefronts)
    bool no_analytic_walk = false;   // YCGE_NO_ANALYTIC_WALK: scenes of analytic objects only are walked by tree_phase's general loop (A/B of analytic_walk; same pixels)
    bool no_walk_tree = false;       // YCGE_NO_WALK_TREE: voxel worlds are walked down the scene tree, leaves and object steps and all (A/B of SceneDev::walk_nodes)
    bool mesh_emit_host = false;     // YCGE_MESH_EMIT_HOST: ycge_scene_upload writes every mesh's records and the treelets on the host, whoever built the trees
    long long mesh_pool_units = 0;   // YCGE_MESH_POOL_UNITS: the capacity (32-byte units of records) the first ycge_scene_attach_meshes re-homes the arena into (0: twice the uploaded records, at least 1 MiB of them)
    long long mesh_pool_max_units = 0;   // YCGE_MESH_POOL_MAX_UNITS: a lower cap on that capacity (0: none; tests provoke the refusal at small size)
    int mesh_emit_device_min = YCGE_MESH_EMIT_DEV_MIN_TRIS_DEFAULT;   // YCGE_MESH_EMIT_DEVICE_MIN: ... and also when no tree built on the device has this many triangles (measured crossover of the whole upload, profiles/mesh_build_rate.json)
    bool no_coop = false;            // YCGE_NO_COOP: no treelets are built, sparse wavefronts keep the regular walk (A/B of the cooperative walk)
    size_t enc_group_bytes = (size_t)256 << 20;   // YCGE_ENC_GROUP_BYTES: raw cells staged per encode group (attach / generate sub-batches); a larger grid is a group of its own
    bool worldgen_host = false;      // YCGE_WORLDGEN_HOST: ycge_scene_generate_grids makes the cells with the host generator (ycge_worldgen.cpp) and sends them up as an attach does
    bool obj_host = false;           // YCGE_OBJ_HOST: ycge_obj_parse reads every file with the host parser (ycge_obj_parse_host's)
    long long obj_device_min = YCGE_OBJ_DEVICE_MIN_DEFAULT;   // YCGE_OBJ_DEVICE_MIN: ... and files of fewer bytes than this (crossover not yet measured)
    bool obj_ground_host = false;    // YCGE_OBJ_GROUND_HOST: ycge_obj_ground takes every held OBJ through the host tail (ycge_obj_ground_host's)
    long long obj_ground_device_min = YCGE_OBJ_GROUND_DEVICE_MIN_DEFAULT;   // YCGE_OBJ_GROUND_DEVICE_MIN: ... and OBJs of fewer triangles than this
    bool obj_ground_phases = false;  // YCGE_OBJ_GROUND_PHASES: a stream synchronise behind every phase of the device tail (ycge_debug_obj_ground_phases: what each costs)
    bool exposure_serial = false;    // YCGE_EXPOSURE_SERIAL: the one-lane chain instead of the chunked exact evaluation
    bool world_store_host = false;   // YCGE_WORLD_STORE_HOST: ycge_world_store_load keeps the world in host memory; its chunks are sliced by a host loop and go up as an attach's cells do
    size_t world_store_slab_bytes = YCGE_WORLD_STORE_SLAB_BYTES_DEFAULT;   // YCGE_WORLD_STORE_SLAB_BYTES: bytes of whole x-planes staged per slab of a load (one plane at least)
    int ws_pool_batch = YCGE_WS_POOL_BATCH_DEFAULT;   // YCGE_WS_POOL_BATCH: records (chunks to materialise, clipped ops, slots) in one launch of the edit pool's kernels, 1..32768
    void read()
    {
        auto geti = [](const char *n, int dflt) { const char *e = getenv(n); return e ? atoi(e) : dflt; };
        if (const char *e = getenv("YCGE_PATH")) path_policy = e[0] == 'w' ? 1 : e[0] == 'm' ? 2 : 0;
        xcd_strips = getenv("YCGE_XCD_STRIPS") != nullptr; generic_walk = getenv("YCGE_GENERIC_WALK") != nullptr;
        no_analytic_walk = getenv("YCGE_NO_ANALYTIC_WALK") != nullptr;
        if (const char *e = getenv("YCGE_PERSIST_MIN_TILES")) persist_min_tiles = atoi(e);
        lpt_always = getenv("YCGE_LPT_ALWAYS") != nullptr;
        no_walk_tree = getenv("YCGE_NO_WALK_TREE") != nullptr; no_lights_beside = getenv("YCGE_NO_LIGHTS_BESIDE") != nullptr; no_flight_stage_overlap = getenv("YCGE_NO_FLIGHT_STAGE_OVERLAP") != nullptr;
        no_lpt = getenv("YCGE_NO_LPT") != nullptr; no_refill = getenv("YCGE_NO_REFILL") != nullptr;
        if (const char *e = getenv("YCGE_WAVE_PROF")) wave_prof_stage = e[0] == 'e' ? 1 : e[0] == 'm' ? 2 : 0;
        if (const char *e = getenv("YCGE_SPLIT")) { split_set = true; split_policy = (uint32_t)strtoul(e, nullptr, 8); }
        split_top_set = getenv("YCGE_SPLIT_TOP") != nullptr || getenv("YCGE_SPLIT_TOP_LG") != nullptr;
        split_top = geti("YCGE_SPLIT_TOP", YCGE_SPLIT_TOP_DEFAULT);
        if (split_top < 0) split_top = 0;
        split_top_lg = geti("YCGE_SPLIT_TOP_LG", 2);
        if (split_top_lg < 1 || split_top_lg > 6) split_top_lg = 2;
        pw_per_cu = geti("YCGE_PW_PER_CU", 32);
        post_band_rows = geti("YCGE_POST_BAND_ROWS", YCGE_POST_BAND_ROWS_DEFAULT); post_k = geti("YCGE_POST_K", YCGE_POST_K_DEFAULT);
        post_groups = geti("YCGE_POST_GROUPS", YCGE_POST_GROUPS_DEFAULT);
        if (post_groups != 8 && post_groups != 16 && post_groups != 32) post_groups = YCGE_POST_GROUPS_DEFAULT;
        split_resolve = geti("YCGE_RES_SPLIT_RESOLVE", 0) != 0;
        taa_copy_guides = geti("YCGE_TAA_COPY_GUIDES", 0) != 0;
        traced_packet = geti("YCGE_TRACED_PACKET", 0) != 0;
        post_mode = geti("YCGE_POST_MODE", 0);
        post_hash = geti("YCGE_POST_HASH_FORM", 0) != 0;
        post_no_split = getenv("YCGE_POST_NO_SPLIT") != nullptr;
        post_probe_band = geti("YCGE_POST_PROBE_BAND", -1);
        post_resident_per_cu = geti("YCGE_POST_RESIDENT", 3);
        post_assume_resident = geti("YCGE_POST_ASSUME_RESIDENT", 0);
        if (post_resident_per_cu < 1 || post_resident_per_cu > 3) post_resident_per_cu = 3;
        post_pad_lds = geti("YCGE_POST_PAD_LDS", 0);
        flight_overlap = geti("YCGE_FLIGHT_OVERLAP", 1) != 0;
        flight_post_gate = geti("YCGE_FLIGHT_POST_GATE", 1) != 0;
        flight_placed_gate = geti("YCGE_FLIGHT_PLACED_GATE", 1) != 0;
        flight_post_pair = geti("YCGE_FLIGHT_POST_PAIR", 1) != 0;
        flight_small_groups = geti("YCGE_FLIGHT_SMALL_GROUPS", 1) != 0;
        flight_priority = geti("YCGE_FLIGHT_PRIORITY", 1);
        flight_no_begin = geti("YCGE_FLIGHT_NO_BEGIN", 0) != 0;
        post_dbg_free = geti("YCGE_POST_DBG_FREE", 0) != 0;
        exposure_serial = getenv("YCGE_EXPOSURE_SERIAL") != nullptr;
        obj_host = getenv("YCGE_OBJ_HOST") != nullptr;
        if (const char *e = getenv("YCGE_OBJ_DEVICE_MIN")) obj_device_min = atoll(e);
        obj_ground_host = getenv("YCGE_OBJ_GROUND_HOST") != nullptr;
        if (const char *e = getenv("YCGE_OBJ_GROUND_DEVICE_MIN")) obj_ground_device_min = atoll(e);
        obj_ground_phases = getenv("YCGE_OBJ_GROUND_PHASES") != nullptr;
        no_coop = getenv("YCGE_NO_COOP") != nullptr;
        res_sched_every = geti("YCGE_RES_SCHED_EVERY", 0);
        bfs_rays = geti("YCGE_BFS", 0);
        if (bfs_rays < 0 || bfs_rays > 64) bfs_rays = 0;
        scene_bvh_host = getenv("YCGE_SCENE_BVH_HOST") != nullptr;
        bvh_waves = geti("YCGE_BVH_WAVES", 16);
        scene_bvh_device_min = geti("YCGE_SCENE_BVH_DEVICE_MIN", YCGE_BVH_DEV_MIN_ITEMS_DEFAULT);
        mesh_bvh_host = getenv("YCGE_MESH_BVH_HOST") != nullptr;
        worldgen_host = getenv("YCGE_WORLDGEN_HOST") != nullptr;
        world_store_host = getenv("YCGE_WORLD_STORE_HOST") != nullptr;
        if (const char *e = getenv("YCGE_WORLD_STORE_SLAB_BYTES")) { const long long v = atoll(e); if (v > 0) world_store_slab_bytes = (size_t)v; }
        ws_pool_batch = geti("YCGE_WS_POOL_BATCH", YCGE_WS_POOL_BATCH_DEFAULT);
        if (ws_pool_batch < 1 || ws_pool_batch > YCGE_WS_POOL_BATCH_DEFAULT) ws_pool_batch = YCGE_WS_POOL_BATCH_DEFAULT;
        if (const char *e = getenv("YCGE_ENC_GROUP_BYTES")) { const long long v = atoll(e); if (v > 0) enc_group_bytes = (size_t)v; }
        mesh_emit_host = getenv("YCGE_MESH_EMIT_HOST") != nullptr;
        if (const char *e = getenv("YCGE_MESH_POOL_UNITS")) { const long long v = atoll(e); if (v > 0) mesh_pool_units = v; }
        if (const char *e = getenv("YCGE_MESH_POOL_MAX_UNITS")) { const long long v = atoll(e); if (v > 0) mesh_pool_max_units = v; }
        mesh_emit_device_min = geti("YCGE_MESH_EMIT_DEVICE_MIN", YCGE_MESH_EMIT_DEV_MIN_TRIS_DEFAULT);
        mesh_bvh_device_min = geti("YCGE_MESH_BVH_DEVICE_MIN", YCGE_MESH_BVH_DEV_MIN_TRIS_DEFAULT);
        mesh_bvh_wide_min = geti("YCGE_MESH_BVH_WIDE_MIN", YCGE_BVH_DEV_MAX_ITEMS);
        if (mesh_bvh_wide_min < 9) mesh_bvh_wide_min = 9;
        if (mesh_bvh_wide_min > YCGE_BVH_DEV_MAX_ITEMS) mesh_bvh_wide_min = YCGE_BVH_DEV_MAX_ITEMS;
    }
};

// One frame's identity from snapshot to commit (TryFlipAndBlit steps 1-3, RaytraceRenderer.cs:159-176): the pose the
// frame is traced with is the pose its reset decision and CommitCamera use.
struct FrameState {
    float pos[3], yaw, pitch, fov;
    bool reset;
    int64_t frame;
    bool scheduled = false;      // the trace ran the single-launch kernel with a longest-first schedule (cost ring in use)
    bool single_launch = false;  // the trace ran the single-launch kernel (its last workgroup stores the placed value), scheduled or not
};

struct MeshHost {
    BuiltTree tree;
};

// The device-side mesh BVH build (ycge_mesh_bvh.cpp drives the kernels of ycge_mesh_bvh_build.hip): its scratch, kept from mesh to mesh of
// one upload and given back when the upload ends, and what it reports about one build.
struct MeshBvhScratch {
    DevBuf<float> tris, items, items_pos;
    DevBuf<uint32_t> ord, ord2, lpref, blk, blk_excl, back_l, hdr, leaf;
    DevBuf<int32_t> node_of, level[2], jobs;
    DevBuf<uint8_t> flag, top, acc, sub_nodes, nodes;
    PinnedBuf stage;
    void release()
    {
        tris.release(); items.release(); items_pos.release(); ord.release(); ord2.release(); lpref.release(); blk.release(); blk_excl.release(); back_l.release();
        hdr.release(); leaf.release(); node_of.release(); level[0].release(); level[1].release(); jobs.release(); flag.release(); top.release(); acc.release();
        sub_nodes.release(); nodes.release(); stage.release();
    }
};
enum { MESH_BVH_BUILT = 0, MESH_BVH_SORT_NO_SPLIT = 1, MESH_BVH_SORT_EMPTY_SIDE = 2, MESH_BVH_TOP_OVERFLOW = 3, MESH_BVH_TOO_DEEP = 4, MESH_BVH_NON_FINITE = 5 };
struct MeshBvhReport {
    int fallback = MESH_BVH_BUILT;     // why the host builds this mesh instead (MESH_BVH_*); Array.Sort at a wide node and a non-finite coordinate are the expected ones
    int wide_nodes = 0, levels = 0, jobs = 0;
    double us = 0.0;                   // items kernel to the tree in host memory
    hipError_t error = hipSuccess;
};

// The arena of an upload assembled on the device (ycge_mesh_bvh.cpp drives the kernels of ycge_mesh_emit.hip): per mesh what the kernels read -
// the buffers of the device-side build taken over from its scratch, or a host-built tree uploaded - and the references of all meshes' nodes.
// Given back when the upload ends, with the builder's scratch.
struct MeshEmit {
    struct Input {
        DevBuf<float> tris;
        DevBuf<uint8_t> nodes;           // RefNode records in pre-order
        DevBuf<uint32_t> leaf;
        DevBuf<int32_t> tri_material;    // empty: `material` for every triangle
        uint32_t n_nodes = 0, n_tris = 0, first_ref = 0;      // first_ref: where its nodes' references start in `refs`
        int32_t material = 0, root_count = 0;                 // root_count: triangles of a leaf root (0: the root is a node)
        bool ready = false;
    };
    std::vector<Input> in;               // one per mesh of the upload (n_nodes == 0: a mesh without triangles)
    DevBuf<uint32_t> refs, tiles, hdr;
    std::vector<uint32_t> hdr_host;      // the last read-back of hdr: [0] units, then per mesh {units, a leaf above 15 triangles, a material out of range, 0}
    uint32_t n_refs = 0;
    double us[3] = {0.0, 0.0, 0.0};      // layout, records, treelets - separated only when asked (mesh_emit_write's `timed`)
    void release() { in.clear(); refs.release(); tiles.release(); hdr.release(); hdr_host.clear(); n_refs = 0; }
};
// mesh `mi` of the upload: built == true takes S.tris / S.nodes / S.leaf of the build that has just made `t`, else `t`, its leaf order and the triangles are uploaded
hipError_t mesh_emit_add(MeshEmit &E, size_t mi, bool built, MeshBvhScratch &S, const BuiltTree &t, const float *tris9, int32_t n_tris, const int32_t *tri_material, int32_t material);
// the builder's scratch and the emit's inputs of ONE upload: kept from mesh to mesh, given back however the upload ends
struct MeshUploadScratch { MeshBvhScratch &s; MeshEmit &e; ~MeshUploadScratch() { s.release(); e.release(); } };
// One mesh's tree by the builder ycge_scene_upload picks: the device's (the same tree byte for byte) from YCGE_MESH_BVH_DEVICE_MIN triangles on - or always, when asked -
// and the host's below that, under YCGE_MESH_BVH_HOST and for what the device builder declines (rep.fallback).  on_device: S holds the tree's triangles, nodes and leaf order.
// d_tris9: the same soup where it already lies on the device (ycge_scene_attach_obj_mesh) - the device builder takes it from there by a device copy; with tris9 null the
// answer is 1, nothing built, wherever the host builder would have to build.
int build_mesh_tree(const Knobs &knobs, bool always_try_device, MeshBvhScratch &S, const float *tris9, int32_t n, hipStream_t stream, BuiltTree &t, bool &on_device, MeshBvhReport &rep,
                    const float *d_tris9 = nullptr);
// The arena of an upload's meshes - records in mesh order, then the treelets unless no_coop - written by the host from the trees (gmeshes[].root_ref), or by the device from
// E's inputs into d_arena at its exact size (root_refs).  YCGE_OK or the error, its text in msg; the three refusals both share are worded in mesh_refusal alone.
int emit_arena_on_host(const std::vector<MeshHost> &trees, const ycge_mesh *meshes, int n_materials, bool no_coop, std::vector<uint8_t> &arena, std::vector<GMesh> &gmeshes, uint32_t &tl_offset, std::string &msg);
int emit_arena_on_device(MeshEmit &E, PinnedBuf &stage, DevBuf<uint8_t> &d_arena, int n_materials, bool no_coop, bool timed, hipStream_t stream, std::vector<uint32_t> &root_refs, uint32_t &tl_offset, std::string &msg);
enum MeshRefusal { MESH_LEAF_ABOVE_15 = 0, MESH_TRI_MATERIAL = 1, MESH_ARENA_FULL = 2 };
int mesh_refusal(MeshRefusal why, int mesh, std::string &msg);          // the refusal's code, its text into msg
// the units of a tree's records as both emits lay them out (a leaf above 15 triangles has none: bad_leaf), and whether its root is a node
uint32_t mesh_tree_units(const BuiltTree &t, bool &bad_leaf);
// E's inputs written into a pooled arena of capacity_units units (tl_offset: its treelet region, 0 none): mesh k's records from unit base_units[k] on (units[k] of
// them, as mesh_tree_units counts), the treelets of exactly these meshes' nodes.  The ranges lie inside the arena and hold zeros.  root_refs on return.
int emit_meshes_into_arena(MeshEmit &E, PinnedBuf &stage, uint8_t *arena, uint32_t capacity_units, uint32_t tl_offset, const std::vector<uint32_t> &base_units, const std::vector<uint32_t> &units,
                           int n_materials, hipStream_t stream, std::vector<uint32_t> &root_refs, std::string &msg);

// The resident voxel grids of a scene (ycge_grid_encode.cpp): the grids of the last ycge_scene_upload keep their indices and its packing;
// ycge_scene_attach_grids takes the lowest free index, a block of the cell arena (size-keyed free list, 256-byte alignment, else the end of
// the arena, which grows geometrically) and a 256-entry region of the LUT; ycge_scene_detach_grids gives index, block and region back.
// Kept by the root context; every device of a multi-device context holds the same layout.
// What a slot needs on the host to turn a (matId, metaId) pair into a cell code (ycge_scene_edit_voxels, ycge_grid_edit.cpp).  A slot
// the device encoded is coded by its lookup table (1 + the first matching entry, n_lookup + 1 for a miss that falls to default_material);
// a slot the host encoded numbers its pairs as they first appeared.  Identical lookup tables are interned (intern_lookup): a world of
// thousands of chunks holds one host copy.
struct LookupTable { std::vector<ycge_voxel_lookup> e; };
struct SlotCodes {
    std::shared_ptr<const LookupTable> lookup;
    int32_t default_material = -1;           // a material of the upload, or -1: a lookup miss has no material
    bool host_encoded = false;
    std::vector<std::pair<int32_t, int32_t>> seen;   // host-encoded: the pairs in code order (code = 1 + index) ...
    std::vector<int32_t> lut;                        // ... and the table that goes with them (entry 0 = -1: empty)
};

struct GridPool {
    std::vector<GGrid> recs;                 // host mirror of d_grids, one per slot (a free slot: zeros)
    std::vector<SlotCodes> codes;            // per slot: how an edit codes a pair (a free slot: empty)
    std::vector<uint8_t> resident;           // per slot: 1 = a grid lives here (a prim may refer to it)
    std::vector<uint32_t> block_bytes;       // per slot: bytes of its block of the cell arena
    std::vector<int32_t> lut_region;         // per slot: first entry of its 256-entry LUT region; -1: the upload's packed entries (not given back)
    std::vector<int32_t> owner;              // per slot: the object of the current Scene.Objects that holds it (-1: none)
    std::set<int32_t> free_index;            // free slots below recs.size()
    std::multimap<uint32_t, uint32_t> free_blocks;   // size -> byte offset
    std::vector<uint32_t> free_luts;
    uint64_t arena_end = 0, lut_end = 0;     // the first byte / entry never handed out
    uint64_t arena_in_use = 0;               // bytes of the resident grids' blocks
    int64_t n_resident = 0, growths = 0, slots_reused = 0, device_encodes = 0, host_encodes = 0;
    bool streamed = false;                   // an attach or a detach has changed the set since the last upload
    double last_attach_us[4] = {0, 0, 0, 0};  // the last attach: copy into the staging, host-to-device copy, encode kernel, read-back
};

// The resident meshes of a scene (ycge_mesh_pool.cpp): the meshes of the last ycge_scene_upload keep their indices and their records, laid
// out exactly as the upload lays them out.  The first ycge_scene_attach_meshes re-homes the arena into an allocation with room -
// [records: `capacity` units][treelets: capacity * YCGE_TL_BYTES_PER_UNIT bytes at the 512-aligned tl_offset] - where a record keeps its
// unit and, the map from a node's unit to its treelet being linear, a treelet keeps its place behind tl_offset.  Kept by the root context;
// every device of a multi-device context holds the same layout.
struct MeshPool {
    MeshRanges ranges;                       // units and indices handed out (ycge_mesh_pool.h)
    std::vector<uint8_t> resident;           // per index: 1 = a mesh lives here (a prim may refer to it)
    std::vector<uint64_t> first_unit;        // per index: where its records start
    std::vector<uint32_t> units;             // per index: units of its records (0: a mesh without triangles)
    bool pooled = false;                     // the arena has been re-homed: capacity / tl_offset describe d_mesh_arena
    bool treelets = false;                   // a pooled arena has a treelet region (not under YCGE_NO_COOP, not behind an upload too large for one)
    uint64_t capacity = 0;                   // units of records the pooled arena has room for
    uint32_t tl_offset = 0;                  // where the treelet region starts: the upload's, then the pooled arena's (0: none)
    int64_t n_resident = 0, units_in_use = 0, growths = 0, device_builds = 0, host_builds = 0;
    double last_attach_us[3] = {0, 0, 0};    // the last attach: the trees, the emit (layout, records, treelets, read-backs), the copies (re-homing, growth, peers)
};

} // namespace ycge_host
using namespace ycge_host;

// what the scene queries of one context hold (ycge_query.cpp): a stream and buffers of their own, made by the first query, grow-only
struct QueryState {
    Stream stream;
    DevBuf<float> rays, hits;
    DevBuf<int32_t> ids;
    DevBuf<uint8_t> occluded;
    DevBuf<uint32_t> first_bad;
    DevBuf<uint64_t> spill;            // [spill levels][resident lanes]
    uint32_t lanes[4] = {0, 0, 0, 0};  // resident lanes of k_query<has_grid, occluded>
    PinnedBuf in_stage, out_stage;
    // ycge_volume_camera_tick (ycge_camera.cpp): k_camera_tick's {input, result} records, its 64 spill columns, their staging
    DevBuf<uint8_t> cam_dev;
    DevBuf<uint64_t> cam_spill;
    PinnedBuf cam_stage;
    // ycge_volume_bodies_tick: k_bodies_tick's {header, n inputs, moves, n results}, its 64 * n spill columns, their staging; grow-only
    DevBuf<uint8_t> bodies_dev;
    DevBuf<uint64_t> bodies_spill;
    PinnedBuf bodies_stage;
};
// one ANSI stream call (ycge_ansi.cpp): the colour form, the console, the viewport, the default colours, the clear-screen prefix; delta: a
// _delta call, which alone reads gap, tolerance (24-bit colour only) and keyframe
// quad: the quadrant-glyph family - 24-bit colour (rgb is set too) with the fitted glyph and colours of k_fit_quadrants under min_contrast
struct AnsiRequest {
    bool rgb = false, quad = false;
    int32_t min_contrast = 0;
    int32_t cw = 0, ch = 0, vx = 0, vy = 0, fg = 0, bg = 0;
    bool clear = false, delta = false;
    int32_t gap = 0, tolerance = 0;
    bool keyframe = false;
};
// One stream call's plan (ycge_ansi.cpp, plan_of): made once a call from its request, the keyframe decision, the framebuffer and whether
// layers are set.  Needs: every ChexelState buffer the call reads or writes, with the size it must have (0: not this call's; ansi_res is
// always 4 words) - ensure_frame_buffers grows the buffers to them, and a frame in flight is queued only onto buffers that meet them already.
// Placement: where the frame's colour plane lies - chexel_encode writes it there and the stream kernels read it there.
struct AnsiPlan {
    bool rgb_palette = false;                          // the default colours' triples (else their indices)
    size_t stream = 0, tile_words = 0;                 // ansi_stream (the bound), ansi_tiles
    size_t held = 0;                                   // delta_held[1 - delta_prev], bytes: the held plane a _delta call writes
    size_t comp = 0, comp_cells = 0, comp_cur = 0;     // each comp_held (bytes), each glyph_held (code units); comp_cur (bytes: a 24-bit layered delta)
    bool frame_in_held = false;                        // the frame's plane lies in delta_held[1 - delta_prev]; else in ChexelState::out, where k_encode_chexels' lie
};
// the console's other framebuffers as the device holds them (ycge_console_set_layers, ycge_ansi.cpp): rect[0..n) bottom first, their cells
// one behind the other - code units, and the colours as k_encode_chexels wrote them for the cells as a cells x 1 framebuffer, in both forms
struct LayerStore {
    int32_t n = 0, raytrace_at = 0;
    uint32_t cells = 0;
    ycge_ansi::LayerRect rect[ycge_ansi::kMaxLayers] = {};
    DevBuf<uint16_t> glyphs;
    DevBuf<uint8_t> pairs, rgba;                       // 2 bytes a cell; 2 * cells RGBA words, the foregrounds then the backgrounds
};
// What one frame hands out: the argument of render_frame_sync / render_frame_in_flight and of everything below them (run_post, chexel_encode,
// chexel_read_back, ansi_enqueue, video_read_sdr).  A value on the entry point's stack, holding borrowed pointers only.  Default-constructed: a
// post stage with no output - nothing to encode, nothing to copy; a NULL pointer to it: no post stage.
// A pageable destination of a SYNCHRONOUS call is redirected into the context's page-locked staging (ycge_ctx::out_stage, ChexelState::stage)
// and noted here; the caller that synchronises the stream calls finish().  The asynchronous entry points refuse pageable destinations ahead
// of their first enqueue, so their value never holds a staged entry: it may leave scope with copies still queued, and its stack lifetime suffices.
struct FrameOutputs {
    float *sdr = nullptr;                              // the caller's destinations: the SDR array ...
    uint8_t *chexels[3] = {nullptr, nullptr, nullptr}; // ... c16, ansi pairs, rgba
    // ycge_render_frame_quadrants: the caller's sub-cell colours (fbW*fbH*12 f32), glyph plane and fitted RGBA plane, any of them NULL
    struct Quadrants { float *sdr; uint16_t *glyphs; uint8_t *rgba; int32_t min_contrast; };
    const Quadrants *quad = nullptr;
    bool quad_colours_ready = false;                   // a video blit: k_video_blit_quadrants wrote ChexelState::quad_sdr already - the encode is the fit alone
    // ycge_render_frame_pixels / _sixel (ycge_sixel.cpp): the caller's per-pixel planes (W x H RGBA words, W x H registers), any of them NULL,
    // and with `stream` set the sixel stream of the registers at the viewport - its bytes are delivered behind the frame's synchronisation
    // A _sixel_delta call: dev_index, the held plane the registers go to in place of SixelState::index, and with dev_prev the plane the
    // terminal shows - the stream is the delta against it (dev_prev NULL: the call's keyframe, the full stream)
    // pal (the _palette calls): 0 the cube's registers; 1 the adaptive palette's, through the palette the context keeps; 2 through a palette
    // built from this picture - the RGBA plane is always written, the registers are k_pal_remap's
    struct Pixels { uint8_t *rgba; uint8_t *index; int32_t dither; bool stream; int32_t vx, vy; bool clear; uint8_t *dev_index = nullptr; const uint8_t *dev_prev = nullptr; int32_t pal = 0; };
    const Pixels *pixels = nullptr;
    const AnsiRequest *ansi = nullptr;                 // the ANSI stream asked for (its encode keeps the pairs - 24-bit colour: the RGBA plane - on the device only)
    bool keyframe = true;                              // ... runs the full stream's kernels (a _delta call: what its DeltaCall decided)
    AnsiPlan plan;                                     // ... and its plan (DeltaCall's)
    uint8_t *dev_stream = nullptr;                     // a frame in flight: the device aliases of the caller's page-locked stream buffer (dev_capacity bytes)
    void *dev_record = nullptr;                        // ... and result record - the stream is delivered by k_ansi_deliver instead of the copy of ansi_res
    size_t dev_capacity = 0;
    struct Staged { void *dst; const void *stage; size_t bytes; } staged[4] = {};
    int n_staged = 0;
    explicit FrameOutputs(float *sdr_ = nullptr, uint8_t *c16 = nullptr, uint8_t *pairs = nullptr, uint8_t *rgba = nullptr) : sdr(sdr_), chexels{c16, pairs, rgba} {}
    // `stage` stands in for the pageable dst in a queued copy
    template <class T> T *redirect(T *dst, void *stage, size_t bytes) { staged[n_staged++] = Staged{dst, stage, bytes}; return static_cast<T *>(stage); }
    // the stream of those copies has been waited for
    void finish() { for (int k = 0; k < n_staged; k++) std::memcpy(staged[k].dst, staged[k].stage, staged[k].bytes); n_staged = 0; }
};
// what the chexel calls of one context hold (ycge_chexel.cpp, ycge_ansi.cpp): filled by the first call.  Nothing of the call at hand: that is its FrameOutputs
struct ChexelState {
    DevBuf<uint8_t> tables;                            // 256 f32 + 256 f64 thresholds
    DevBuf<uint8_t> out[2];                            // the encoded bytes, per post parity (as d_sdr / d_sdr2)
    DevBuf<float> quad_sdr;                            // the quadrant calls: k_tonemap_quadrants' 12 floats a chexel ...
    DevBuf<uint16_t> quad_glyphs;                      // ... and k_fit_quadrants' code units (its RGBA plane lies in out[], where k_encode_chexels' does)
    PinnedBuf stage;                                   // page-locked staging of pageable destinations (synchronous calls only)
    // the ANSI stream calls (ycge_ansi.cpp; kernels: ycge_ansi.hip, ycge_ansi_rgb.hip): the stream's buffers
    DevBuf<uint8_t> ansi_stream;                       // the stream (its bound)
    DevBuf<uint32_t> ansi_tiles;                       // per-tile byte counts, then offsets (a delta: four words a tile)
    DevBuf<unsigned long long> ansi_res;               // {length, changed, emitted, run starts}, as the scan wrote them (the full stream: the length alone)
    DevBuf<float> ansi_palette;                        // the 16 palette colours as 8 SDR chexels, then their 16 ANSI indices (bytes at float 48)
    bool ansi_palette_ready = false;
    PinnedBuf ansi_res_host;                           // page-locked words ansi_res is copied to
    // The _delta calls: delta_held[delta_prev] holds what the last stream handed out left on the terminal while delta_valid, for the stream
    // delta_key names - the frame's pairs, or in 24-bit colour the plane the terminal displays; a call with any other key (the other colour
    // form, another family, another geometry, layers set or not) finds no valid state.  The encode of a 256-colour _delta call writes its
    // pairs into delta_held[1 - delta_prev]; in 24-bit colour a keyframe's encode writes the plane there and a delta's write kernel writes
    // emitted ? cur : shown (AnsiPlan::frame_in_held).  A successful call flips delta_prev - nothing is copied.  Whatever shows the terminal
    // something else (a plain _ansi call, ycge_resize, a failure) clears delta_valid.
    DevBuf<uint8_t> delta_held[2];
    int delta_prev = 0;
    bool delta_valid = false;
    // {rgb, quad (the quadrant family, whose held state is the composite's alone), layered (layers were set), cw, ch, vx, vy, dfg, dbg, fbW, fbH}
    using DeltaKey = std::array<int32_t, 11>;
    DeltaKey delta_key{};
    DevBuf<uint8_t> rgb_palette;                       // RGB8 of the 16 palette colours: the encoder's 8 x 2 RGBA plane of ansi_palette's chexels
    bool rgb_palette_ready = false;
    // Layers (ycge_console_set_layers): while layers.n > 0 every stream is that of the console-wide composite.  comp_held / glyph_held
    // [delta_prev] hold the composite the last _delta stream left on the terminal, the call at hand composes into [1 - delta_prev] and a
    // successful _delta call flips them with delta_held.  A 24-bit delta composes into comp_cur instead, and its write kernel fills
    // comp_held[1 - delta_prev] with emitted ? cur : shown.  Kept across ycge_resize and ycge_scene_upload.
    LayerStore layers;
    DevBuf<uint8_t> comp_held[2], comp_cur;
    DevBuf<uint16_t> glyph_held[2];
    // Frames in flight (ycge_render_frame_async_ansi): the stream buffers are one set per context, so a frame's encode .. deliver follows the
    // deliver of the frame before: flight_ev is recorded behind every k_ansi_deliver, on flight_stream, and waited for in front of the next
    // encode on another stream while flight_pending (join_async clears it).  flight_sticky: the word a deliver sets when the stream exceeds
    // the capacity (join_async).
    Event flight_ev;
    hipStream_t flight_stream = nullptr;
    bool flight_pending = false;
    PinnedBuf flight_sticky;
};
// what the sixel calls of one context hold (ycge_sixel.cpp; kernels: ycge_sixel.hip): made by the first call, grow-only
struct SixelState {
    DevBuf<uint8_t> rgba, index;                       // k_sixel_pixels' / k_video_pixels' planes of the frame at hand (the planes calls and the plain _sixel calls)
    // The _sixel_delta calls, frames and video alike: held[held_prev] is the register plane of the last sixel stream handed out, while
    // ChexelState::delta_valid holds and ChexelState::delta_key names the sixel family ({kSixelFamily, 0, 0, W, H, vx, vy, 0, 0, fbW, fbH}) -
    // one terminal, one delta state.  A call's registers go to held[1 - held_prev]; a successful call flips held_prev, nothing is copied.
    // No other call writes either plane
    DevBuf<uint8_t> held[2];
    int held_prev = 0;
    static constexpr int32_t kSixelFamily = 2;         // DeltaKey[0] (the ANSI families: rgb, 0 or 1)
    DevBuf<uint32_t> span;                             // k_sixel_diff's spans: lo[bands], hi[bands]
    DevBuf<uint32_t> last1, lines, line_bytes, meta;   // the encoder's per-(band, colour) widths, its line list, the lines' bytes then offsets, the line count
    DevBuf<uint8_t> header, stream;                    // the stream's parts 1 to 5 as the host built them, and the stream (its bound)
    std::array<int32_t, 5> header_key{{0, 0, 0, 0, 0}}; // {W, H, vx, vy, clear} the header on the device was built for (W = 0: none)
    uint32_t header_bytes = 0;
    DevBuf<unsigned long long> res;                    // the stream's length as k_sixel_scan wrote it ...
    PinnedBuf res_host;                                // ... and the page-locked word it is copied to
    PinnedBuf stage;                                   // page-locked staging of pageable destinations
    // The adaptive palette (the _palette calls; kernels: ycge_sixel_palette.hip): the histogram, and the palette block - the kept palette
    // (bin-to-box table, register definitions, n; layout: ycge_sixel_host.h) while pal_kept.  Independent of geometry: ycge_resize keeps it,
    // frames and video share it; a failure behind a _palette call's refusals drops it.  pal_prefix: the stream's parts 1 to 4 on the device
    DevBuf<uint32_t> pal_hist;
    DevBuf<uint8_t> pal_block, pal_prefix;
    bool pal_kept = false;
    std::array<int32_t, 5> pal_prefix_key{{0, 0, 0, 0, 0}};
    uint32_t pal_prefix_bytes = 0;
};
// what the video blits of one context hold (ycge_video.cpp): made by the first blit, grow-only; nothing a ray-traced frame reads
struct VideoState {
    int32_t key[5] = {0, 0, 0, 0, 0};                  // {src_w, src_h, fbW, fbH, ss} the tables were made for
    DevBuf<uint8_t> tables;                            // int32 x0[hiW], f32 wx[hiW][6], int32 y0[hiH], f32 wy[hiH][6]
    DevBuf<uint8_t> frame;                             // the source frame
    DevBuf<float> sdr;                                 // its chexels {top rgb, bottom rgb}
    PinnedBuf stage;                                   // page-locked staging of a pageable source frame
    int64_t table_builds = 0;
};
// the OBJ a context holds (ycge_obj_parse, ycge_obj.cpp): one at a time, whoever parsed it; nothing a frame reads
struct ObjState {
    bool held = false;
    int32_t n_positions = 0, n_triangles = 0, on_device = 0;
    int64_t n_lines = 0;
    DevBuf<float> positions, triangles;                // 3 per vertex; the last ycge_obj_triangles' soup, 9 per triangle
    DevBuf<int32_t> faces;                             // 3 per triangle
    DevBuf<uint8_t> header;                            // what the kernels report (ObjHeader, ycge_obj.hip)
    PinnedBuf stage;                                   // page-locked staging of a pageable text, one chunk at a time
    float used_min[3] = {0, 0, 0}, used_max[3] = {0, 0, 0};   // the box of the vertices any face uses
    int64_t device_parses = 0, host_parses = 0, last_decline = 0;
    double last_us[3] = {0, 0, 0};                     // lines + classify + scans; token parsing + used / range / bounds; the last triangle pass
    // ycge_obj_ground (ycge_obj_ground.hip): union-find parents, faces and first face per root, the three term planes, the chosen component's vertices
    DevBuf<uint32_t> ground_parent, ground_count, ground_first;
    DevBuf<float> ground_terms;
    DevBuf<uint8_t> ground_used, ground_header;
    int64_t ground_device_tails = 0, ground_host_tails = 0, ground_last_decline = 0, ground_rounds = 0;
    double ground_last_us = 0;
    double ground_phase_us[5] = {0, 0, 0, 0, 0};       // YCGE_OBJ_GROUND_PHASES: labelling, count + winner, terms, the three sums, bounds + read-back
};

// the VG01 world a context holds (ycge_world_store_load, ycge_world_store.cpp): one at a time, not scene state - ycge_scene_upload keeps it.
// Every device of a multi-device context holds the cells; the rest is the root's.
struct WorldStore {
    bool held = false, on_host = false;                // on_host: YCGE_WORLD_STORE_HOST, the cells are host_cells
    ycge::WsShape shape{};
    DevBuf<int32_t> d_cells;                           // the payload in VG01 order, on this context's device
    std::vector<int32_t> host_cells;
    std::vector<uint8_t> occupied;                     // per chunk, (cx, cy, cz) with cx outermost: 1 when a cell has mat != 0
    int64_t bytes = 0, slabs = 0;                      // of the last load
    double load_us[3] = {0, 0, 0};                     // ... its copies into the staging (wall), its host-to-device copies and occupancy kernels (stream time, root device)
    std::vector<Event> slice_ev;                       // begin / end of the last attach's slice launches on the root's stream, a pair per group (kept from attach to attach)
    size_t slice_ev_used = 0;
    int64_t device_chunks = 0, host_chunks = 0;        // chunks sliced by k_ws_slice (made by k_wp_fill, a fields store) / by the host, since the context was made
    // ycge_world_store_generate, YCGE_WORLD_STORE_FIELDS: no cells anywhere - d_fields holds the WpFields of the window (wp_layout,
    // ycge_worldgen_cells.h) with the anyLeaves flags settled, and a chunk or a plane is made from them when it is asked for
    bool fields = false;
    DevBuf<uint8_t> d_fields;                          // on this context's device
    ycge::wg::World gen_world{};
    ycge::wg::Window gen_window{};
    double last_fill_us = 0;                           // the last attach's k_wp_fill launches on the root (wall: launch to stream idle)
    // the last generate (root): form asked for, 1 when the host generator made it (the knobs), anyLeaves passes, plane slabs, then
    // microseconds: field kernels, anyLeaves pass loop, occupancy + read-back, plane kernels (CELLS form; stream time), the host generator
    int64_t gen_form = -1, gen_on_host = 0, gen_passes = 0, gen_slabs = 0;
    double gen_us[5] = {0, 0, 0, 0, 0};
    // ycge_world_store_reserve_edits, a fields store: the pool of materialised chunks.  d_pool is this context's device's; the map is the root's.
    DevBuf<uint8_t> d_pool;                            // pool_cap slots of pool_stride bytes: a chunk's S^3 cells as k_wp_fill writes them
    size_t pool_stride = 0;
    int32_t pool_cap = 0, pool_used = 0;
    std::vector<int32_t> slot_of;                      // per chunk (occupied's order): its slot, or -1
    std::vector<int32_t> chunk_in;                     // per slot: its chunk, or -1
    std::vector<uint8_t> gen_occupied;                 // per chunk: what the generate found (occupied follows the edits)
};

struct ycge_ctx {
    ycge_config cfg;
    Knobs knobs;
    std::string err;
    int device = 0;
    // one process, several GPUs (config.n_devices >= 2): this context is rank 0 and owns one context per further device
    std::vector<ycge_ctx *> peers;
    ycge_ctx *parent = nullptr;
    Event pushed_ev;                           // a peer's tiles have arrived in the parent's frame buffers
    // config.multi_device_exchange = YCGE_EXCHANGE_RCCL (root only): the in-process communicators (ncclCommInitAll over devices[]), rank r's
    // on device r's stream; exchange_mode says what the frames really use (0 = peer push: not asked for, or librccl.so / its symbols absent)
    int exchange_mode = 0;
    std::vector<void *> nccl_comms;
    DevBuf<float> all_slabs;                   // every context of an RCCL frame: the gathered slabs of all ranks (the root un-permutes its copy)
    // A peer's share of a frame is ISSUED by a thread of its own (trace launches, tile push, event): eight devices driven one after the
    // other from the caller's thread would put 7 x ~0.1 ms of launch calls in front of the last device's first kernel - as long as
    // the frame itself.  The worker sleeps between frames; the root posts a frame, issues its own share, then collects the peers'.
    struct PeerWorker {
        std::thread th;
        std::mutex m;
        std::condition_variable cv;
        int job = 0;                           // 0 idle, 1 frame posted, 2 done, -1 quit
        FrameState fs{};
        int rc = 0;
    };
    std::unique_ptr<PeerWorker> worker;
    std::deque<FrameState> pending;            // frames traced by ycge_trace_tiles and not yet resolved (pipelined callers)
    hipStream_t last_stream = nullptr;         // the stream the last tiled call ran on (scene updates wait for it too)
    Stream stream;
    Event ev[4];
    // a side stream, forked from and joined to the frame's stream: the next frame's schedule, the light loop beside the next round's
    // trace (stage pipeline), the resident ring's schedules and the static A-trous weights run on it
    Stream side_stream;
    Event side_ev[2];
    Event traced_ev, order_ev;   // the next frame's schedule is built on the side stream, beside TAA
    bool order_pending = false;
    char device_name[256] = {0};
    int compute_units = 0;

    // geometry of the trace grid
    int fbW = 0, fbH = 0, ss = 1, hiW = 0, hiH = 0;
    int tiles_x = 0, tiles_y = 0, n_tiles = 0, n_owned = 0, tiles_per_rank_padded = 0;

    // camera (lock(camLock), RaytraceRenderer.cs:142-147)
    std::mutex cam_lock;
    float cam_pos[3] = {0.0f, 1.0f, 0.0f};
    float yaw = 0.0f, pitch = 0.0f, fov_deg = 45.0f;

    int64_t frame_counter = 0;                 // RaytraceRenderer.cs:24
    // TemporalAA camera memory (TemporalAA.cs:11-15) and history validity
    float last_cam[3] = {NAN, NAN, NAN}, last_yaw = NAN, last_pitch = NAN;
    bool taa_valid = false;

    // per-pixel buffers in HBM (row-major, x + y*hiW)
    DevBuf<float> current_hdr, g_albedo, g_normal, g_depth, taa_hist, prev_normal, prev_depth;
    DevBuf<uint8_t> sky, prev_sky;
    // TAA's guide planes are the last resolved frame's normal, depth and sky flag.  The synchronous single-device frame does not copy them
    // (17 of the 87 bytes TAA moved per pixel): it keeps the planes the trace wrote and traces the next frame into a second set (g2_*: swapped
    // with g_normal / g_depth / sky before that trace, so those names are always the newest frame's).  guide_prev_*: the planes that hold
    // the last resolved frame's guides - a frame's own planes after such a frame, null = prev_normal / prev_depth / prev_sky after a frame
    // of the copying forms (frames in flight, tiled and tile-resident frames, multi-device frames; YCGE_TAA_COPY_GUIDES=1), which
    // are the only users of prev_* and allocate them (guides_copying).  Nothing may write the planes guide_prev_* name before the TAA that
    // reads them has run: whoever writes g_normal / g_depth / sky first calls guides_keep.
    DevBuf<float> g2_normal, g2_depth;
    DevBuf<uint8_t> g2_sky;
    const float *guide_prev_normal = nullptr, *guide_prev_depth = nullptr;
    const uint8_t *guide_prev_sky = nullptr;
    // tiled frame: the trace writes its tiles here (same full-frame indexing), ycge_resolve_gathered writes the buffers above -
    // so the trace of frame N+1 may run beside the all-gather and resolve of frame N (two streams, caller-ordered)
    DevBuf<float> t_hdr, t_albedo, t_normal, t_depth;
    DevBuf<uint8_t> t_sky;
    // frames in flight (ycge_render_frame_async): the trace of frame N + 1 runs beside the TAA of frame N, so a frame's trace outputs
    // alternate between the five buffers above and these (swapped before the trace: the names above are always the newest frame's)
    DevBuf<float> alt_hdr, alt_albedo, alt_normal, alt_depth;
    DevBuf<uint8_t> alt_sky;
    DevBuf<float> alt2_hdr, alt2_albedo, alt2_normal, alt2_depth;      // (three sets: the trace of frame N + 1 must not wait for the TAA of frame N - 1, which finds
    DevBuf<uint8_t> alt2_sky;                                          //  its places among frame N's wavefronts late; it waits for TAA of frame N - 2)
    int set_id[3] = {0, 1, 2};                     // which of the three sets the names current / alt / alt2 hold
    Stream taa_stream, stream2;      // stream2: the traces of odd frames in flight (two traces may overlap: the tail of one, the bulk of the next)
    DevBuf<uint64_t> stack_spill2;                 // ... which then need a traversal-stack spill area of their own
    uint64_t *spill_override = nullptr;            // set around trace_frame by ycge_render_frame_async
    Event flight_fork_ev;
    SignalWord placed_flag;                        // signal memory: the number of the newest frame in flight whose trace has placed its last workgroup
    uint32_t placed_expect = 0, placed_next = 0;   // what the next trace waits for (0: nothing) / the value the next trace stores
    uint64_t placed_waits = 0;                     // traces queued behind a placed value so far (ycge_flight_query)
    // frames in flight WITH the post stage (ycge_render_frame_async_sdr): post of frame N beside the traces and TAA of the frames after it
    Event flight_taa_ev, post_hist_ev, post_done_ev, post_set_ev[3];
    bool post_hist_pending = false, post_busy = false, post_set_pending[3] = {false, false, false};
    Event tile_trace_ev[2];      // tiled frames: the trace (and slab pack) of the newest frame of each parity is done
    bool tile_trace_used[2] = {false, false};
    Event set_resolved_ev[3];
    bool set_read[3] = {false, false, false};             // a TAA launch on taa_stream has read this set: the next trace into it waits for set_resolved_ev
    int out_set = 0;                               // which set the names above hold
    bool async_outstanding = false;
    // ... and their schedules: the one for frame N + 1 is built WHILE frame N is traced, from the costs up to frame N - 1 (a frame
    // staler than the synchronous path's, which builds it between the two traces), into the buffers frame N is not reading
    DevBuf<uint32_t> flight_order[3], flight_ws[3];         // (frames in flight use all three, by frame number mod 3; tiled frames two, by parity)
    int64_t flight_order_frame[3] = {-1, -1, -1};  // the frame number each buffer's schedule was built for (-1: none)
    Event flight_order_ev[3];     // the schedule in each buffer is complete (side stream)
    int64_t last_frame_deferred = -2;              // the newest tiled frame whose trace was followed by a deferred schedule
    bool in_flight_taa = false;                    // taa_and_commit is called by ycge_render_frame_async with two traces overlapping: one-wavefront workgroups
    bool in_flight_call = false;                   // trace_frame is called by ycge_render_frame_async
    std::vector<Event> flight_ev;             // begin / end of the trace launches of the frames in flight, a ring (ycge_async_trace_times)
    uint64_t flight_frames = 0;                    // queued since the last ycge_async_trace_times
    // ---- tile-resident form (one process per GPU; ycge_trace_tiles_resident / ycge_resolve_tiles_resident): TAA on this rank's own tiles
    // with a one-pixel halo of {hdr, sky} exchanged between the ranks, the history never leaves its rank; a ring of K frame sets so that K
    // tiled traces may be in flight (a rank's launch is its longest chains: its period per frame becomes max(slot time, chain / K))
    struct ResidentSet {
        DevBuf<float> hdr, normal, depth;
        DevBuf<uint8_t> sky;
        DevBuf<uint64_t> spill;
        Event traced, resolved;
        bool traced_used = false, resolved_used = false;
    };
    std::vector<ResidentSet> rsets;
    // ycge_trace_tiles_resident_batch: the frames of a batch leave their launch parameters here instead of launching (trace_frame), one
    // launch traces them all (the records travel as its arguments)
    bool batch_collect = false;
    std::vector<FrameParams> batch_P;
    std::vector<TraceOut> batch_O;
    static constexpr int kBatchMax = YCGE_TRACE_BATCH_MAX;
    DevBuf<uint64_t> batch_spill[2];               // a spill area as wide as the batch's frames together, per batch parity: two batches may run at a time
    uint64_t batch_count = 0;
    Event batch_done[2];                           // a batch's launch: the batch after the next may scratch its spill area after it
    bool batch_spill_used[2] = {false, false};
    static constexpr uint32_t kResCostFrames = 16; // the resident ring's own cost ring: K - 1 slots are being written, one is cleared, the rest are read
    DevBuf<uint32_t> res_cost;
    // three schedule buffers taken in turn: one is built behind the trace of every R-th frame M (R = the ring's depth; YCGE_RES_SCHED_EVERY) and
    // serves the frames from M + K on - a trace never waits for a trace younger than frame N - K - until a newer one does
    std::vector<DevBuf<uint32_t>> res_order, res_ws;
    std::vector<Event> res_order_ev, res_order_read_ev;
    std::vector<int64_t> res_order_frame;          // per buffer: the frame M its schedule was built behind (-1: none)
    int res_order_next = 0;                        // the buffer the next build writes
    Event res_last_traced;          // stage-pipeline scenes share their queues between frames: their traces follow each other
    bool res_last_traced_used = false;
    std::vector<int64_t> halo_send_counts, halo_recv_counts;          // records (4 floats) per peer rank
    DevBuf<uint32_t> d_halo_send_px, d_halo_recv_px;
    DevBuf<uint32_t> d_halo_index;             // [pixel of the frame] place of its halo record in the receive buffer (pixels other ranks own that border this rank's tiles; others: unused) - k_resolve_tiles
    bool halo_ready = false;
    DevBuf<float> dbg_rays, dbg_hit_t;
    DevBuf<int32_t> dbg_prim, dbg_sub;
    DevBuf<uint64_t> dbg_rng;
    DevBuf<unsigned long long> counters, wave_prof, dbg_counters;
    DevBuf<float> own_slab;                    // used when world_size > 1 and the caller passes no slab
    // wavefront pipeline storage (ycge_kernels.hip: QEntry / HitRec / LEntry), sized for one ray per pixel
    DevBuf<uint8_t> wf_q0, wf_q1, wf_hit, wf_lq;
    DevBuf<uint32_t> wf_seg;                      // segment counter of the persistent extend stage
    DevBuf<uint32_t> wf_counts, tile_order;
    // the stage pipeline's second set (frames in flight: two voxel-world traces at a time, ycge_render_frame_async): queues, counters, both spill areas
    DevBuf<uint8_t> wf2_q0, wf2_q1, wf2_hit, wf2_lq;
    DevBuf<uint32_t> wf2_seg, wf2_counts;
    DevBuf<uint64_t> stack_spill_side2;
    // denoise / exposure / tonemap stage (ycge_post.hip), allocated on the first frame that asks for SDR output
    DevBuf<float> den_a, den_b, unit_n, exp_terms, d_sdr, d_sdr2;      // d_sdr2: SDR frames in flight read back one array while the next frame's tonemap fills the other
    DevBuf<float> atrous_statw;                // [pixel][25 taps][3]: colour-independent weight factors of an in-place A-trous iteration
    DevBuf<uint8_t> exp_scratch;                  // chunk records of the exposure sum (k_exposure_sum)
    DevBuf<uint32_t> post_progress;               // k_atrous_stream: levels published per band, one 128-byte line each
    uint32_t post_epoch = 0;                      // ... counted from here in the next launch
    uint32_t post_ticket = 0;                     // k_atrous_stream, bands in order of arrival: numbers drawn so far (the counter lives in post_progress)
    // a second set of everything the denoiser scratches, for the post stages of every other frame in flight: two of them run side by side
    // (each is a dependent chain that leaves the chip idle); the exposure state passes from one to the next in frame order
    struct PostSet { DevBuf<float> den_a, den_b, unit_n, exp_terms, atrous_statw; DevBuf<uint8_t> exp_scratch; DevBuf<uint32_t> post_progress; uint32_t post_epoch = 0, post_ticket = 0;
                     void release() { den_a.release(); den_b.release(); unit_n.release(); exp_terms.release(); atrous_statw.release(); exp_scratch.release(); post_progress.release(); post_epoch = post_ticket = 0; } } alt_post;
    int post_resident_seen[2] = {-1, -1};         // post_resident_per_cu: the runtime's answer for the whole-band / split-band instantiation (-1: not asked yet)
    DevBuf<uint8_t> tone_state;                   // ToneMapper state; lives as long as the context (not reset by Resize)
    struct InplaceSchedule { int w = 0, h = 0, step = 0, levels = 0, bands = 0, rows_per_band = 0, levels_per_launch = 0; uint32_t max_level_pixels = 0, window_width = 0; bool split = false; DevBuf<uint32_t> pixels, offsets, pass_level; DevBuf<int32_t> band_desc; };
    std::vector<std::unique_ptr<InplaceSchedule>> schedules; // level schedules of the in-place A-trous iterations, by (w, h, step)
    // what ycge_scene_update_objects needs from the last full upload
    std::vector<GMesh> gmeshes_host;
    std::vector<std::array<float, 6>> grid_bounds;   // VolumeGrid.TryGetBounds per grid; max < min marks an empty grid
    std::vector<std::array<float, 7>> grid_solid;    // GGrid::solid_lo / solid_hi per grid (copied into the grid's object record: the walk culls before it enters)
    int n_materials = 0, max_mesh_depth = 0;
    bool materials_can_mirror = false;
    bool has_dynamic_textures = false;           // Scene.HasDynamicTextures: every frame restarts the TAA history (RaytraceRenderer.cs:171)
    const float *denoised = nullptr;              // result of the last post stage (one of den_a / den_b / taa_hist)
    DevBuf<uint32_t> block_cost, block_order, order_ws;   // k_trace scheduling feedback (4 blocks of 8x8 px per tile)
    DevBuf<uint32_t> cost_snap;                    // a schedule built while traces are in flight reads a copy of the cost ring (ycge_launch_order_blocks)
    bool block_order_valid = false;
    DevBuf<uint64_t> stack_spill;                 // [YCGE_TRAVERSAL_STACK - 12][persistent lanes]
    bool any_light_lit = false;                   // some light has a contribution (GLight::dark == 0): the timed light loop has shadow rays to trace
    DevBuf<uint64_t> stack_spill_side;            // ... of the stage kernel that runs on the side stream beside another (the light loop beside the next round's trace)
    DevBuf<float> path_stack;                  // [3][11][persistent lanes], only for scenes with transparent materials
    int spill_levels = 0;                      // traversal depth beyond the 12 LDS levels, from the uploaded trees
    int wf_rounds = 2;                         // 2 = primary + diffuse bounce; 4 when a surface can mirror (<= 2 mirror bounces)
    bool has_grid = false;

    // scene
    bool have_scene = false;
    SceneDev sd{};
    DevBuf<GNode> d_scene_nodes;
    DevBuf<GNode> d_walk_nodes;        // SceneDev::walk_nodes (worlds of voxel grids): the scene nodes + YCGE_WALK_LEAF_NODES entries per leaf child
    DevBuf<int32_t> d_grid_owner;      // SceneDev::grid_owner
    int walk_scene_nodes = 0;          // scene nodes the walk tree was made from (0: SceneDev::walk_nodes is null)
    DevBuf<uint8_t> d_mesh_arena;
    DevBuf<uint32_t> d_scene_leaf;
    DevBuf<GPrim> d_prims;
    DevBuf<GMaterial> d_materials;
    DevBuf<GMesh> d_meshes;
    DevBuf<GGrid> d_grids;
    GridPool grid_pool;                // (root context)
    MeshPool mesh_pool;                // (root context)
    bool pending_transparent = false, pending_textured = false;          // (root) of ycge_scene_append_materials: SceneDev's flags follow with the next install of the objects
    std::map<std::string, std::weak_ptr<const LookupTable>> lookup_tables;   // (root) the interned lookup tables of the resident grids, by their bytes
    std::vector<ycge_prim> last_prims;  // (root) the object list the last ycge_scene_upload / ycge_scene_update_objects accepted: an edit that changes a held grid's record installs it again
    // ycge_scene_attach_grids: the batch's descriptors, results, lookup tables and raw cells in page-locked memory (root) and on this
    // device; encoded bytes that wait for the arena to grow
    PinnedBuf enc_stage;
    DevBuf<uint8_t> d_enc_in, d_enc_out;
    // ycge_scene_generate_grids (ycge_worldgen_scene.cpp): the column records of the batch's distinct (cx, cz) on this device, then their keys and tops
    DevBuf<uint8_t> d_wg_cols;
    int64_t worldgen_device_chunks = 0, worldgen_host_chunks = 0;          // since the context was made (root)
    int worldpregen_last_passes = 0;                                      // ycge_scene_generate_world's last call on the root: anyLeaves passes,
    double worldpregen_last_us[4] = {0, 0, 0, 0};                         // ... field kernels, anyLeaves passes, tops, fill kernels
    double worldgen_last_us[2] = {0, 0};                                  // the last call on the root: column kernel, fill + tree kernels
    DevBuf<uint8_t> d_cells;
    DevBuf<int32_t> d_lut;
    DevBuf<uint32_t> d_tex_pixels;             // textures of YCGE_MAT_TEXTURED materials
    // a live texture's next frame travels through page-locked staging (two buffers taken in turn) and a stream-ordered copy on the
    // context's stream: behind the traces that still read the old frame, ahead of the ones queued after the call
    PinnedBuf tex_stage[2];
    Event tex_stage_ev[2];
    // GPU -> host copies never target memory whose mapping the library does not control (copy_out below): page-locked staging of its own
    PinnedBuf out_stage;
    Event tex_order_ev;         // "everything queued on the second trace stream so far": a live texture's copy waits for it
    bool tex_stage_busy[2] = {false, false};
    int tex_stage_next = 0;
    DevBuf<int32_t> d_tex_info;
    std::vector<int32_t> tex_info_host;        // {first word, width, height, flags} per texture (ycge_scene_update_texture)
    DevBuf<GLight> d_lights;
    BuiltTree scene_tree;                      // host copy of the scene BVH in the reference's format (ycge_read_accel)
    bool scene_tree_on_device = false;         // ... not fetched yet from the last device-side build (accel_view does it on demand)
    int32_t dev_tree_nodes = 0, dev_tree_items = 0;
    DevBuf<float> d_bvh_items;                 // device-side scene BVH build (ycge_bvh_build.hip): item boxes + centroids, nine planes
    DevBuf<uint8_t> d_bvh_scratch, d_bvh_ref, d_bvh_res;
    int64_t bvh_device_builds = 0, bvh_host_fallbacks = 0, bvh_host_builds = 0;
    double bvh_last_build_us = 0.0;
    std::vector<MeshHost> meshes;
    MeshBvhScratch mesh_bvh;                   // device-side mesh BVH builds of the upload at hand
    MeshEmit mesh_emit;                        // ... and its arena, when that is assembled on the device
    int64_t mesh_emit_dev_meshes = 0, mesh_emit_host_meshes = 0, mesh_emit_arena_bytes = 0;       // of the last upload: meshes whose records the device / the host wrote
    double mesh_emit_last_us = 0.0;            // the last device emit: layout, records, treelets, their two read-backs
    int64_t mesh_bvh_device_builds = 0, mesh_bvh_host_builds = 0, mesh_bvh_host_fallbacks = 0;       // since the context was made
    int64_t mesh_bvh_sorts = 0, mesh_bvh_depth = 0, mesh_bvh_wide_nodes = 0, mesh_bvh_jobs = 0;       // of the last upload: summed / deepest over its meshes
    double mesh_bvh_last_us = 0.0;
    // scene queries (ycge_scene_hit / ycge_scene_occluded, ycge_query.cpp): a stream and buffers of their own, made by the first query;
    // scene_ev marks the device work of the last scene change on `stream` - a query waits for it and for nothing a frame queued after it
    std::unique_ptr<QueryState> query;
    Event scene_ev;
    // device chexel colours (ycge_render_frame_chexels / _async_chexels, ycge_chexel.cpp): the encoded buffers per post parity, the
    // threshold tables, the staging of pageable destinations
    ChexelState chexels;
    SixelState sixel;            // the sixel presenter (ycge_render_frame_pixels / _sixel, ycge_sixel.cpp)
    VideoState video;            // Video mode (ycge_video_blit, ycge_video.cpp)
    ObjState obj;                // the parsed OBJ (ycge_obj_parse, ycge_obj.cpp)
    WorldStore world_store;      // the resident VG01 world (ycge_world_store_load, ycge_world_store.cpp)

    ycge_ctx() = default;
    ycge_ctx(const ycge_ctx &) = delete;
    ycge_ctx &operator=(const ycge_ctx &) = delete;
    ~ycge_ctx();                 // ycge_host.cpp: what has an ORDER (worker, communicators, peers, the streams' drain); the members free themselves
    void stop_worker();          // a peer's issuing thread: told to quit and joined
    void drain();                // waits for every stream of this context, with its device current

    int fail(int code, const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define HIP_TRY(ctx, call)                                                                                   \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) return (ctx)->fail(e_ == hipErrorOutOfMemory ? YCGE_ERR_OUT_OF_MEMORY : YCGE_ERR_DEVICE, \
                                                 "%s failed: %s", #call, hipGetErrorString(e_));            \
    } while (0)

#define YCGE_FLIGHT_RING 1024u       // frames in flight whose trace launches keep their timing events (ycge_async_trace_times)

extern "C" void ycge_peer_worker_main(ycge_ctx *root, ycge_ctx *peer);      // ycge_frame.cpp: a peer device's thread (ycge_create starts it)
// ---- what the other translation units of the library call in ycge_host.cpp and ycge_scene.cpp (defined there, in this namespace)
namespace ycge_host {
struct H3 { float x, y, z; };
H3 h_norm(H3 a);                // ycge_host.cpp: a / |a| (a zero vector stays)
int morton3(int x, int y, int z);          // ycge_host.cpp: a voxel's place in its 8 x 8 x 8 brick (VolumeGrid.cs:246-252)
// where a trace of the tile-resident form writes and which schedule it follows (trace_frame's last argument)
struct ResidentTarget {
    ycge_ctx::ResidentSet *set;
    uint32_t *cost;                 // this frame's slot of the resident cost ring
    const uint32_t *order, *n_order;        // the schedule built for this frame (null: blocks in index order)
};
// librccl.so, dlopen'ed on first use (the library does not link it: a host without RCCL loses nothing but this option).  An instance the
// process already holds - bench.py's torch.distributed brings its own - is preferred over loading a second one.
struct RcclApi {
    void *h = nullptr;
    int (*CommInitAll)(void **comms, int ndev, const int *devlist) = nullptr;
    int (*CommDestroy)(void *comm) = nullptr;
    int (*AllGather)(const void *send, void *recv, size_t count, int dtype, void *comm, hipStream_t stream) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool ok = false, tried = false;
};
const RcclApi &load_rccl();
size_t slab_floats(const ycge_ctx *c);
bool host_memory_is_page_locked(const void *p, size_t bytes);
// how one post stage runs (run_post's last argument; the defaults: a synchronous frame nobody times)
struct PostRun {
    bool timed = false;                  // ev[3] is recorded behind the encode (the caller asked for statistics)
    hipEvent_t history_read = nullptr;   // recorded once the TAA history has been read for the last time
    hipEvent_t before_copy = nullptr;    // recorded in front of the read-back: the exposure state is this frame's
    hipEvent_t tone_wait = nullptr;      // the frame before has left its exposure state: waited for in front of this frame's exposure step
    bool second_sdr = false;             // into the second device SDR array and set of encoded bytes (frames in flight, by parity)
    bool second_set = false;             // on the second set of denoise buffers (post stages side by side)
};
int run_post(ycge_ctx *c, hipStream_t stream, FrameOutputs &out, const PostRun &run);     // ycge_post_host.cpp: steps 6-8, the encode and the read-backs `out` asks for
int join_async(ycge_ctx *c);
// TemporalBlendWithClamp's parameters from the raw config values (RaytraceRenderer.cs:218, :305): every TAA launch - the frames', the
// tile-resident resolve's, ycge_test_taa's - is handed what this makes
inline ycge::TaaParams taa_params(int w, int h, float taa_alpha, int taa_clamp_radius, float taa_luminance_pad, bool reset)
{
    ycge::TaaParams T;
    T.w = w; T.h = h;
    T.alpha = cs_max(0.0f, cs_min(1.0f, taa_alpha));      // :305
    T.radius = taa_clamp_radius > 0 ? taa_clamp_radius : 0;
    T.pad_lum = taa_luminance_pad;
    T.reset = reset ? 1 : 0;
    return T;
}
int check_post_probe(ycge_ctx *c, const char *fn, bool any_rank = false);       // ycge_post_host.cpp: who may be probed (any_rank: a rank of several too)
int guides_keep(ycge_ctx *c, bool *swapped = nullptr);       // in front of anything that writes g_normal / g_depth / sky: the last resolved frame's guides are not among them afterwards
void guides_unkeep(ycge_ctx *c);              // ... undone: the frame failed, the names stay with the last frame that was rendered
int guides_copying(ycge_ctx *c, ycge::TaaGuides &in, ycge::TaaGuidesOut &out);       // the guide arguments of a TAA launch of the copying forms (call guides_copied behind the launch)
inline void guides_copied(ycge_ctx *c) { c->guide_prev_normal = c->guide_prev_depth = nullptr; c->guide_prev_sky = nullptr; }
void guides_forget(ycge_ctx *c);              // new frame size: no guides, no planes
int copy_out(ycge_ctx *c, void *dst, const void *src, size_t bytes);
int fill_stats(ycge_ctx *c, ycge_frame_stats *st, const FrameState &fs, bool did_reset, bool have_taa, double wall_ms);
int quiesce(ycge_ctx *c);
inline std::vector<ycge_ctx *> contexts_of(ycge_ctx *c) { std::vector<ycge_ctx *> v{c}; v.insert(v.end(), c->peers.begin(), c->peers.end()); return v; }          // root, then peers
inline int quiesce_all(ycge_ctx *c) { for (ycge_ctx *x : contexts_of(c)) { const int rc = quiesce(x); if (rc != YCGE_OK) return rc; } return YCGE_OK; }
// one step on the root, then on each peer: stops at the first failure, and a peer's error text is the root's (the caller reads it there)
template <class Step> int on_root_then_peers(ycge_ctx *c, Step step)
{
    int rc = step(c);
    for (ycge_ctx *p : c->peers) { if (rc != YCGE_OK) break; rc = step(p); if (rc != YCGE_OK) c->err = p->err; }
    return rc;
}
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
// room for `need` elements with the first `keep` preserved (device to device): the one place that copies resident bytes (the grid pool's tables)
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
inline double us_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
// the calling thread's current device goes back to the root's on every way out (a failed step on a peer's device included)
struct DeviceGuard { int device; explicit DeviceGuard(int d) : device(d) {} ~DeviceGuard() { (void)hipSetDevice(device); } };
void release_resident(ycge_ctx *c);
int query_hit_batch(ycge_ctx *c, const char *fn, const float *rays, int32_t n, float *hits, int32_t *ids);   // ycge_query.cpp: ycge_scene_hit's batch under another export's name
int alloc_tile_buffers(ycge_ctx *c);          // ycge_host.cpp: queue segments, hit records, spill columns (for c->spill_levels) and schedules of the owned tiles
void snapshot_frame(ycge_ctx *c, FrameState &fs);
void schedule_policy(const ycge_ctx *c, uint32_t &policy, uint32_t &split_top, int resident_ring = 0, bool batched = false);
int scene_is_flat(const ycge_ctx *c);
bool frame_is_single_launch(const ycge_ctx *c);
bool should_reset_history(const ycge_ctx *c, const float pos[3], float yaw, float pitch);
void fill_frame_params(ycge_ctx *c, ycge::FrameParams &P, int64_t frame, const float pos[3], float yaw, float pitch, float fov_deg);
int trace_frame(ycge_ctx *c, float *d_slab, hipStream_t stream, FrameState &fs, bool timed, hipEvent_t launch_begin = nullptr, hipEvent_t launch_end = nullptr, const ResidentTarget *rt = nullptr);
int validate_grid(const ycge_grid &g, int gi, int n_materials, std::string &msg);          // ycge_scene.cpp: one grid's argument checks
void grid_record_init(const ycge_grid &g, GGrid &G);                                       // ... its record from the arguments (clamps, cull_t_limit)
void grid_record_solid(GGrid &G, const int lo[3], const int hi[3], uint64_t brick_mask);   // ... and from the solid voxels' index box
std::array<float, 6> grid_world_bounds(const ycge_grid &g);
int encode_grid_host(ycge_ctx *c, const ycge_grid &g, int gi, int n_materials, const GGrid &G, uint8_t *cells, std::vector<int32_t> &lut, int lo[3], int hi[3],
                     uint64_t &brick_mask, std::vector<std::pair<int32_t, int32_t>> *seen_out = nullptr);   // the host encoder (first-seen codes; seen_out: the pairs in code order)
// ycge_mesh_pool.cpp: the pool's view of an upload (every mesh of it resident in mesh order, nothing free), what the next install of the objects publishes,
// and the bodies of ycge_scene_attach_meshes / _detach_meshes / _append_materials / ycge_debug_mesh_pool_stats (arguments checked there)
void mesh_pool_reset(ycge_ctx *c, uint32_t tl_offset);
void mesh_pool_publish(ycge_ctx *c);
int scene_attach_meshes(ycge_ctx *c, const ycge_mesh *meshes, int32_t n, int32_t *out_mesh_index);
int scene_attach_device_soup(ycge_ctx *c, const float *d_tris9, int32_t n_triangles, int32_t material, int32_t *out_mesh_index);   // one mesh whose soup lies on the root's device
int scene_detach_meshes(ycge_ctx *c, const int32_t *mesh_index, int32_t n);
int scene_append_materials(ycge_ctx *c, const ycge_material *materials, int32_t n, int32_t *out_first_index);
int mesh_pool_stats(ycge_ctx *c, int64_t *out12);
void flatten_material(const ycge_material &m, GMaterial &g, bool &any_transparent, bool &any_textured);          // ycge_scene.cpp: one material's device record
void grid_pool_reset(ycge_ctx *c, const std::vector<GGrid> &recs, size_t arena_bytes, size_t lut_entries, std::vector<SlotCodes> codes = {});   // ycge_grid_encode.cpp: after an upload
// ycge_grid_edit.cpp: how edits code the pairs of grid g (a grid of `root`'s scene; lut: a host-encoded grid's table, entry 0 first), the interned copy of a lookup table,
// and the bodies of ycge_scene_edit_voxels / ycge_world_store_edit's argument checks
SlotCodes slot_codes_of(ycge_ctx *root, const ycge_grid &g, int n_materials, const std::vector<std::pair<int32_t, int32_t>> *seen, const int32_t *lut);
std::shared_ptr<const LookupTable> intern_lookup(ycge_ctx *root, const ycge_voxel_lookup *lookup, int32_t n);
int scene_edit_voxels(ycge_ctx *c, const ycge_voxel_edit *ops, int32_t n, uint32_t *out_info);
int update_objects(ycge_ctx *c, const ycge_prim *prims, int32_t n_prims);          // ycge_scene.cpp: the body of ycge_scene_update_objects (arguments checked)
// Where the raw cells of an attach's grids come from (attach_grids_from, ycge_grid_encode.cpp: the body of ycge_scene_attach_grids for any source; arguments checked by the callers, n >= 1, all or
// nothing).  Host-made cells are written into the staging of their group and go up with it; device-made cells are written on every device where k_grid_encode reads them: only descriptors and tables go up.
struct CellSource {
    bool on_device = false;          // the cells are made by fill(), not by write()
    bool caller_cells = false;       // ycge_grid.cells are the cells, readable throughout the call (else: never read; a pair with no material is named when its group ends)
    bool foreign_cells = false;      // not the caller's, yet arbitrary (a world file's): a grid whose cells missed the lookup table has its distinct pairs counted, as the caller's are
    size_t group_max = SIZE_MAX;     // grids in one group
    virtual ~CellSource() = default;
    // the cells of grid k, 2 * nx * ny * nz int32 in ycge_grid.cells order: into its group's staging, or for the host encoder (a lookup table k_grid_encode does not take)
    virtual int write(ycge_ctx *root, size_t k, const ycge_grid &g, int32_t *cells) = 0;
    // device-made: the bytes of launch records the source wants on the device ahead of the cells of a group of m grids (at d_head), and the launch on x's
    // stream that writes the cells of grid group[j] to d_cells[j].  x == root: waits, refuses what came out wrong and hands the cells to the caller if asked
    virtual size_t head_bytes(size_t /* m */) const { return 0; }
    // how a refusal names cell `cell` (ycge_grid.cells order; kNoCell: the grid as a whole) of grid k when the cells are not the caller's
    static constexpr uint32_t kNoCell = 0xffffffffu;
    virtual std::string where(size_t k, uint32_t /* cell */) const { return "grid " + std::to_string(k); }
    virtual int fill(ycge_ctx * /* root */, ycge_ctx * /* x */, const std::vector<int> & /* group */, uint8_t * /* d_head */, const std::vector<int32_t *> & /* d_cells */) { return YCGE_OK; }
};
int attach_grids_from(ycge_ctx *c, const ycge_grid *grids, int32_t n, int32_t *out_grid_index, CellSource &src);
int query_scene_changed(ycge_ctx *c);       // ycge_query.cpp: record scene_ev behind a scene upload / objects update
int chexel_encode(ycge_ctx *c, hipStream_t stream, const FrameOutputs &asked, const float *d_sdr, bool second);   // ycge_chexel.cpp: run_post's encode behind the tonemap (a no-op unless chexels or a stream are asked for)
int chexel_read_back(ycge_ctx *c, hipStream_t stream, FrameOutputs &out, bool second);   // ... and its copies behind the SDR read-back
int render_frame_sync(ycge_ctx *c, FrameOutputs *out, ycge_frame_stats *st);             // ycge_frame.cpp: ycge_render_frame (out NULL: no post stage; finished when it returns)
int check_in_flight(ycge_ctx *c);                                                        // ycge_frame.cpp: the contexts and configurations the frames in flight refuse
int check_post_frame(ycge_ctx *c);                                                       // ycge_frame.cpp: ... and a presenter's frame with the post stage
int render_frame_in_flight(ycge_ctx *c, FrameOutputs *out);                              // ycge_frame.cpp: ycge_render_frame_async(_sdr)
void halo_layout(int hiW, int hiH, int rank, int world, std::vector<int64_t> &send_counts, std::vector<int64_t> &recv_counts, std::vector<uint32_t> &send_px, std::vector<uint32_t> &recv_px);
int check_quadrant_call(ycge_ctx *c, const char *fn, int32_t min_contrast);              // ycge_chexel.cpp: what every quadrant call refuses - an odd super_sample, min_contrast outside 0..255
int ensure_tables(ycge_ctx *c, ChexelState &X);                                           // ycge_chexel.cpp: LinearToSrgb8's thresholds on the device, once
int sixel_encode(ycge_ctx *c, hipStream_t stream, const FrameOutputs &asked);            // ycge_sixel.cpp: asked.pixels' kernels behind the tonemap (chexel_encode hands them on) ...
int sixel_read_back(ycge_ctx *c, hipStream_t stream, FrameOutputs &out);                 // ... and the copies of its planes and of the stream's length (chexel_read_back)
// ... the bodies of ycge_sixel_stream_bound, ycge_sixel_encode_host (no context), ycge_render_frame_pixels, ycge_render_frame_sixel and the two hooks
int sixel_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes);
int sixel_encode_host(const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len);
int sixel_frame_pixels(ycge_ctx *c, float *out_top_bottom_sdr, uint8_t *out_rgba, uint8_t *out_index, int32_t dither, ycge_frame_stats *st);
int sixel_frame_stream(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t dither, uint8_t *out_stream, size_t capacity,
                       size_t *out_len, float *out_top_bottom_sdr, ycge_frame_stats *st);
int sixel_test_pixels(ycge_ctx *c, const float *hdr, int32_t fbW, int32_t fbH, int32_t ss, float exposure, int32_t dither, uint8_t *out_rgba, uint8_t *out_index);
int sixel_test_stream(ycge_ctx *c, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len);
// ... and of the delta and video forms: ycge_sixel_encode_delta_host (no context), ycge_render_frame_sixel_delta, ycge_video_blit_pixels, ycge_video_blit_sixel
// (keyframe < 0) and ycge_video_blit_sixel_delta, and their two hooks
int sixel_encode_delta_host(const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity, size_t *out_len,
                            uint32_t *out_info);
int sixel_frame_stream_delta(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream,
                             size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st);
int sixel_video_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, float *out_top_bottom_sdr, uint8_t *out_rgba, uint8_t *out_index,
                       int32_t dither);
int sixel_video_stream(ycge_ctx *c, const char *fn, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t viewport_x, int32_t viewport_y,
                       int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                       float *out_top_bottom_sdr);
int sixel_test_video_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t fbW, int32_t fbH, int32_t ss, int32_t dither,
                            uint8_t *out_rgba, uint8_t *out_index);
int sixel_test_delta_stream(ycge_ctx *c, const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity,
                            size_t *out_len, uint32_t *out_info);
// ... and of the adaptive palette's: ycge_sixel_palette_stream_bound, the two host functions (no context), the frame and video calls (frame NULL: a
// traced frame; out_stream NULL: the planes call) and the two hooks
int sixel_palette_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes);
int sixel_palette_host(const uint8_t *rgba, int32_t W, int32_t H, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count);
int sixel_encode_palette_host(const uint8_t *index, const uint8_t *pct, int32_t count, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out,
                              size_t capacity, size_t *out_len);
int sixel_frame_palette(ycge_ctx *c, const char *fn, bool stream, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t hold, uint8_t *out_stream,
                        size_t capacity, size_t *out_len, uint8_t *out_rgba, uint8_t *out_index, uint8_t *out_palette, int32_t *out_count, float *out_top_bottom_sdr,
                        ycge_frame_stats *st);
int sixel_video_palette(ycge_ctx *c, const char *fn, bool stream, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t viewport_x, int32_t viewport_y,
                        int32_t clear_screen, int32_t hold, uint8_t *out_stream, size_t capacity, size_t *out_len, uint8_t *out_rgba, uint8_t *out_index,
                        uint8_t *out_palette, int32_t *out_count, float *out_top_bottom_sdr);
int sixel_test_palette(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t hold, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count);
int sixel_test_palette_stream(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, int32_t hold, uint8_t *out, size_t capacity,
                              size_t *out_len);
int ansi_enqueue(ycge_ctx *c, hipStream_t stream, const FrameOutputs &out, const uint8_t *d_plane);   // ycge_ansi.cpp: out.ansi's stream kernels behind the encode on the frame's plane (where out.plan puts it), and the length's copy
// ycge_video.cpp: Video mode.  The refusals of a source frame; upload + k_video_blit on `stream` for a geometry (*d_sdr: its SDR array);
// the SDR read-back (a pageable array: staged as run_post does it); the test hooks' bodies
int video_check_frame(ycge_ctx *c, const char *fn, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp);
int video_enqueue(ycge_ctx *c, hipStream_t stream, const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const float **d_sdr,
                  DevBuf<float> *quad_sdr = nullptr, bool blit = true);          // blit false: the upload and the tables alone (k_video_pixels' frame without an SDR)
int video_read_sdr(ycge_ctx *c, hipStream_t stream, const float *d_sdr, FrameOutputs &out);
int video_host_tables(int32_t src_w, int32_t src_h, int32_t fbW, int32_t fbH, int32_t ss, int32_t *x0, float *wx, int32_t *y0, float *wy, float *geom3);
int video_test_blit(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t fbW, int32_t fbH, int32_t ss, float *sdr_out,
                    float *quad_out = nullptr);
// ycge_obj.cpp: MeshLoader.FromObj from file bytes - the bodies of ycge_obj_parse_host (no context), ycge_obj_parse / _read / _triangles / _release and ycge_debug_obj_stats
int obj_parse_host(const uint8_t *text, size_t bytes, float *positions, int32_t *faces, ycge_obj_info *info, char *msg, size_t msg_bytes);
int obj_parse(ycge_ctx *c, const uint8_t *text, size_t bytes, ycge_obj_info *info);
int obj_read(ycge_ctx *c, float *positions, int32_t *faces);
int obj_triangles(ycge_ctx *c, int32_t normalize, float target_size, float scale, const float translate[3], float *out_triangles, float out_bounds[6]);
int obj_release(ycge_ctx *c);
int obj_stats(ycge_ctx *c, int64_t *out6);
// ... and MeshScenes.AddMeshAutoGround on the held OBJ: the bodies of ycge_obj_ground_host (no context), ycge_obj_ground, ycge_obj_triangles_auto_ground and their hooks
int obj_ground_host(const float *positions, int32_t n_positions, const int32_t *faces, int32_t n_triangles, ycge_obj_ground_info *out);
int obj_ground(ycge_ctx *c, ycge_obj_ground_info *out);
int obj_triangles_auto_ground(ycge_ctx *c, float scale, const float target[3], float *out_triangles, float out_bounds[6], ycge_obj_ground_info *out_info);
int obj_attach_mesh(ycge_ctx *c, int32_t auto_ground, int32_t normalize, float target_size, float scale, const float translate_or_target[3], int32_t material,
                    int32_t *out_mesh_index, float out_bounds[6]);          // ... and of ycge_scene_attach_obj_mesh
int obj_ground_stats(ycge_ctx *c, int64_t *out6);
int obj_ground_phases(ycge_ctx *c, int64_t *out5);
// ycge_world_store.cpp: the bodies of ycge_world_file_info (no context), ycge_world_store_load / _info / _release, ycge_scene_attach_world_chunks and the hooks
int world_file_info(const uint8_t *bytes, size_t n_bytes, int32_t dims_out[3], size_t *payload_offset_out, char *msg, size_t msg_bytes);
int world_store_load(ycge_ctx *c, const int32_t *cells, int32_t nx, int32_t ny, int32_t nz, int32_t chunk_size);
int world_store_info(ycge_ctx *c, int32_t dims_out[3], int32_t *chunk_size_out, uint8_t *occupied_out, size_t capacity);
int world_store_release(ycge_ctx *c);
int world_store_attach(ycge_ctx *c, const int32_t *keys, int32_t n, const ycge_grid *proto, int32_t *out_grid_index);
int world_store_chunk(ycge_ctx *c, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t dims_out[3]);
int world_store_stats(ycge_ctx *c, int64_t *out8);
// ... and of ycge_world_store_generate (the generator as the store's source), ycge_world_store_read and ycge_debug_world_store_generate_stats
int world_store_generate(ycge_ctx *c, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t form);
int world_store_read(ycge_ctx *c, int32_t x0, int32_t planes, int32_t *cells_out);
int world_store_generate_stats(ycge_ctx *c, int64_t *out9);
int world_store_edit(ycge_ctx *c, const ycge_voxel_edit *ops, int32_t n);          // ... and of ycge_world_store_edit
// ... and of the pool of materialised chunks beside a fields store: ycge_world_store_reserve_edits / _edit_slots / _revert_chunks
int world_store_reserve_edits(ycge_ctx *c, int32_t max_chunks);
int world_store_edit_slots(ycge_ctx *c, int32_t *capacity_out, int32_t *used_out);
int world_store_revert_chunks(ycge_ctx *c, const int32_t *keys, int32_t n);
} // namespace ycge_host
