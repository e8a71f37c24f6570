/* ycge_hooks.h - what libycge_hip.so exports BESIDE the drop-in boundary (include/ycge.h).
 *
 * NOT part of the boundary: nothing here is bound by the C# host (bindings/csharp/), nothing here is covered by
 * YCGE_ABI_VERSION, any of it may change between builds.  These are the handles tests/ and profiles/ hold the
 * library by - the host-side builders and schedules called WITHOUT a GPU (the CPU suite compares them with the
 * oracle node for node), read-outs of profiling instantiations, fault and layout probes - plus a few functions that
 * cross from the host translation units into the kernel ones (csrc/*.cpp -> csrc/*.hip).  The kernel launchers
 * themselves (ycge_launch_*: one per kernel, plain C linkage so that the host .cpp files need no HIP compiler) are
 * exported as well and are not listed one by one.  tests/test_host_cpu.py holds this list to `nm -D` of the library.
 */
#ifndef YCGE_HOOKS_H
#define YCGE_HOOKS_H

#include "ycge.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- layout probe: sizeof the C structs as the library was compiled (0 ycge_vec3, 1 material, 2 prim, 3 mesh, 4 voxel_lookup, 5 grid,
 * 6 light, 7 scene, 8 config, 9 frame_stats, 10 flight_info, 11 world) - the ctypes and C# mirrors are held to it */
size_t ycge_abi_sizeof(int32_t which);

/* ---- host-side builders and schedules, no GPU needed (tests/test_host_cpu.py: against the oracle, bit for bit) */
/* Objects/BVH.cs:258-459 (flavour 0) / MeshBVH.cs:371-576 (flavour 1) over given boxes and centroids; returns the node count */
int ycge_host_build_tree(const float *bounds, const float *centroids, int32_t n, int32_t flavour, void *nodes_out, int32_t *leaf_out,
                         int32_t *stats_out /* [root, max_depth, sort_fallbacks] */);
int ycge_host_build_mesh(const float *tris9, int32_t n, void *nodes_out, int32_t *leaf_out, int32_t *stats_out);
/* the device records of one mesh as ycge_scene_upload lays them out (64-byte nodes, 96-byte triangle pairs; with the cooperative walk's treelets) */
int ycge_host_mesh_arena(const float *tris9, int32_t n, void *out, int64_t capacity_bytes, uint32_t *root_ref_out);
int ycge_host_mesh_arena_treelets(const float *tris9, int32_t n, void *out, int64_t capacity_bytes, uint32_t *root_ref_out, uint32_t *tl_offset_out);
/* the in-place A-trous iteration's level schedule (RaytraceRenderer.cs:718), its bands, the row-parity split, the LDS window's width */
int ycge_host_inplace_schedule(int32_t w, int32_t h, int32_t step, uint32_t *pixels_out, uint32_t *offsets_out, int32_t capacity);
int ycge_host_inplace_bands(int32_t w, int32_t h, int32_t step, int32_t rows_per_band, uint32_t *entries_out, int64_t entries_capacity,
                            uint32_t *offsets_out, int64_t offsets_capacity, int32_t *info_out);
int ycge_host_split_bands(int32_t w, int32_t h, int32_t step, int32_t *row_band_out, int32_t *desc_out, int32_t desc_capacity, int32_t *max_px_out);
int ycge_host_band_window_width(int32_t w, int32_t h, int32_t step, int32_t rows_per_band, int32_t K, int32_t G);
/* the halo lists of the tile-resident form (what ycge_halo_counts counts), rank by rank */
int ycge_host_halo_layout(int32_t hiW, int32_t hiH, int32_t rank, int32_t world, int64_t *send_counts, int64_t *recv_counts,
                          uint32_t *send_px, uint32_t *recv_px, int64_t capacity);

/* ---- device chexel colours (csrc/ycge_chexel.cpp): LinearToSrgb8's thresholds as the library computed them with the C library's pow -
 * entry k - 1 the smallest binary32 / binary64 whose byte is >= k (255 each; host only) - and the encode kernel on caller-given SDR
 * values (w x h chexels of {top rgb, bottom rgb}; NULL outputs are skipped; layouts as ycge_render_frame_chexels) */
int ycge_host_srgb_thresholds(float *f32_out, double *f64_out);
int ycge_test_encode_chexels(ycge_ctx *c, const float *sdr, int32_t w, int32_t h, uint8_t *c16, uint8_t *ansi, uint8_t *rgba);
/* ---- the ANSI escape stream (csrc/ycge_ansi.cpp): its kernels alone on caller-given ANSI pairs (fbW x fbH {fg, bg}, any values 0..255),
 * with the geometry, defaults, refusals and output of ycge_render_frame_ansi */
int ycge_test_ansi_stream(ycge_ctx *c, const uint8_t *pairs, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x,
                          int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                          size_t *out_len);
/* ---- the delta ANSI stream (csrc/ycge_ansi.cpp, kernels csrc/ycge_ansi.hip): the delta kernels alone on caller-given pair arrays,
 * prev_pairs and pairs both fbW x fbH {fg, bg}, with the rules, refusals and out_info of ycge_render_frame_ansi_delta.  A NULL prev_pairs
 * (or clear_screen != 0) gives the keyframe, the bytes of ycge_test_ansi_stream.  Stateless: pair buffers of its own, the context's delta
 * state untouched */
int ycge_test_ansi_delta(ycge_ctx *c, const uint8_t *prev_pairs, const uint8_t *pairs, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                         int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                         uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info);
/* ---- the 24-bit colour streams (csrc/ycge_ansi.cpp, kernels csrc/ycge_ansi_rgb.hip): the stream kernels alone on a caller-given colour
 * image in the layout they read in the product - out_rgba's, fbW x 2 fbH RGBA8, row 2 cy the top half-cell, the fourth byte ignored - with
 * the geometry, defaults and refusals of ycge_render_frame_ansi_rgb / _rgb_delta.  The delta hook is stateless: shown (NULL or
 * clear_screen != 0: the keyframe, ycge_test_ansi_rgb_stream's bytes) and cur are the caller's, and out_shown (or NULL) receives the next
 * shown in the same layout with every fourth byte 255 - cur after a keyframe, otherwise cur where a covered cell was emitted and shown
 * everywhere else - so a test chains frames without a scene */
int ycge_test_ansi_rgb_stream(ycge_ctx *c, const uint8_t *rgba, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x,
                              int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                              size_t *out_len);
int ycge_test_ansi_rgb_delta(ycge_ctx *c, const uint8_t *shown, const uint8_t *cur, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                             int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                             int32_t tolerance, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, uint8_t *out_shown);
/* ---- the layered streams (csrc/ycge_ansi.cpp, kernels csrc/ycge_ansi_cells.hip.h): the compose kernel and the stream kernels alone on a
 * caller-given framebuffer plane (rgb == 0: fbW x fbH pairs; else the fbW x 2 fbH RGBA plane), n >= 1 layers as ycge_console_set_layers
 * takes them, and an optional previous composite - prev_colours in the plane's own form for a console_w x console_h framebuffer, prev_glyphs
 * console_w * console_h code units.  delta == 0: the full stream (out_info untouched).  delta != 0: the rules and out_info of the _delta
 * calls; a NULL prev_colours / prev_glyphs or clear_screen != 0 gives the keyframe.  tolerance is read when rgb != 0 alone.  out_colours /
 * out_glyphs (or NULL) receive the next composite in the same forms: this call's, and in a 24-bit delta cur where a cell was emitted and
 * prev elsewhere (every fourth byte 255).  Stateless: the context's own layers, request and delta state are untouched */
int ycge_test_ansi_layers(ycge_ctx *c, int32_t rgb, const uint8_t *plane, int32_t fbW, int32_t fbH, const ycge_console_layer *layers, int32_t n,
                          int32_t raytrace_at, const uint8_t *prev_colours, const uint16_t *prev_glyphs, int32_t console_w, int32_t console_h,
                          int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t delta,
                          int32_t merge_gap, int32_t tolerance, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                          uint8_t *out_colours, uint16_t *out_glyphs);
/* ---- the quadrant-glyph frames (csrc/ycge_chexel.cpp, csrc/ycge_ansi.cpp; the rules: ycge.h at ycge_render_frame_quadrants).
 * ycge_test_quadrant_sdr: k_tonemap_quadrants alone on a caller-given hi-res buffer hdr (fbH*2*ss rows of fbW*ss pixels, 3 f32 each) with the
 * effective exposure `exposure`, whatever the context's framebuffer is; out fbW*fbH*12 f32.  ss even, 2..64.  Touches no frame state.
 * ycge_test_quadrant_fit: k_fit_quadrants alone on n cells of 12 f32 as an n x 1 framebuffer: out_glyphs n code units, out_rgba n foreground
 * words then n background words (either NULL, not both).
 * ycge_test_ansi_quad_stream / _delta: the quadrant streams' kernels alone on caller-given planes of the fbW x fbH framebuffer - glyphs,
 * fbW*fbH code units (none of them ' '), and rgba, fbW x 2 fbH RGBA8 with row 2 cy the foreground - with the geometry, defaults and refusals
 * of ycge_render_frame_ansi_quad / _quad_delta and no layers.  The delta hook is stateless: shown_colours (console_w x 2 console_h RGBA8) and
 * shown_glyphs (console_w*console_h code units) are the composite the terminal shows - either NULL, or clear_screen != 0: the keyframe,
 * ycge_test_ansi_quad_stream's bytes - and out_shown_colours / out_shown_glyphs (or NULL) receive the next such, every fourth byte 255 */
int ycge_test_quadrant_sdr(ycge_ctx *c, const float *hdr, int32_t fbW, int32_t fbH, int32_t ss, float exposure, float *out);
int ycge_test_quadrant_fit(ycge_ctx *c, const float *quad_sdr, int32_t n, int32_t min_contrast, uint16_t *out_glyphs, uint8_t *out_rgba);
int ycge_test_ansi_quad_stream(ycge_ctx *c, const uint16_t *glyphs, const uint8_t *rgba, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                               int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream,
                               size_t capacity, size_t *out_len);
int ycge_test_ansi_quad_delta(ycge_ctx *c, const uint8_t *shown_colours, const uint16_t *shown_glyphs, const uint16_t *glyphs, const uint8_t *rgba, int32_t fbW,
                              int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16,
                              int32_t clear_screen, int32_t merge_gap, int32_t tolerance, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                              uint8_t *out_shown_colours, uint16_t *out_shown_glyphs);
/* ---- the delivery of a stream with frames in flight (csrc/ycge_ansi.cpp, kernel csrc/ycge_ansi_flight.hip): k_ansi_deliver alone.  src
 * (n_src bytes) is uploaded as the device stream and {length, counts[0..3)} as the words the scan writes; the kernel then copies into
 * out_stream (capacity bytes, page-locked, 16-byte aligned) and fills out_result (page-locked, 8-byte aligned), and the call synchronises.
 * keyframe != 0: the record of a full stream, {1, 0, 0, 0}, whatever the counts.  groups > 0: that many workgroups, so that the
 * grid-stride wrap is reached at small sizes; 0: the product's grid.  length > capacity: nothing is copied, status = 1, and the next call
 * on the context that joins (ycge_wait) fails once with YCGE_ERR_DEVICE.  Refused: frames in flight on the context, a length within the
 * capacity but above n_src, what ycge_render_frame_async_ansi refuses of the two buffers */
int ycge_test_ansi_deliver(ycge_ctx *c, const uint8_t *src, size_t n_src, uint64_t length, size_t capacity, int32_t keyframe, const uint32_t *counts,
                           int32_t groups, uint8_t *out_stream, ycge_ansi_async_result *out_result);
/* ---- Video mode (csrc/ycge_video.cpp).  ycge_host_video_tables: host only, no device - for src_w x src_h -> fbW x fbH ss the tables
 * k_video_blit reads, as the library computed them with the C library's sinf: per hi-res column x0 (hiW = fbW*ss entries) and its six
 * normalised weights (6 hiW), per hi-res row y0 (hiH = fbH*2*ss) and weights (6 hiH), and {scale, offX, offY} (VideoRenderer.cs:75-81).
 * ycge_test_video_blit: the kernel alone on a caller-given geometry, whatever the context's framebuffer is; sdr_out fbW*fbH*6 f32.
 * ycge_test_video_blit_quadrants: k_video_blit_quadrants alone likewise, ss even; sdr_out as there, quad_out fbW*fbH*12 f32 {TL, TR, BL, BR} */
int ycge_host_video_tables(int32_t src_w, int32_t src_h, int32_t fbW, int32_t fbH, int32_t ss, int32_t *x0_out, float *wx_out, int32_t *y0_out,
                           float *wy_out, float *geometry_out);
int ycge_test_video_blit(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t fbW, int32_t fbH, int32_t ss,
                         float *sdr_out);
int ycge_test_video_blit_quadrants(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t fbW, int32_t fbH,
                                   int32_t ss, float *sdr_out, float *quad_out);
/* ---- the post stage (csrc/ycge_post_host.cpp, csrc/ycge_post.hip) on caller-given inputs.  state_out = 6 words: {aeExposure, effective exposure} as
 * binary32, the chunks k_exposure_sum added one by one, 0, the frame's logSum as binary32, its counted samples.
 * ycge_test_post_stage: hist / albedo / normal hiW*hiH*3 f32, depth hiW*hiH f32, sky hiW*hiH u8 are copied over the context's TAA history and
 * G-buffer, ae_in over its exposure state, and the frames' own run_post runs on them (knobs, schedules, side stream as in a frame);
 * denoised_out hiW*hiH*3 (may be NULL), sdr_out fbW*fbH*6.  It dirties those buffers and the exposure state.  Refused, the context left as it
 * was: frames in flight, a peer or multi-device context, a rank of several.
 * ycge_test_exposure: the exposure sum kernels alone on n terms (0 = a skipped sample), serial != 0 the one-lane form; touches no context state */
int ycge_test_post_stage(ycge_ctx *c, const float *hist, const float *albedo, const float *normal, const float *depth, const uint8_t *sky, float ae_in,
                         float *denoised_out, float *sdr_out, uint32_t *state_out);
int ycge_test_exposure(ycge_ctx *c, const float *terms, int64_t n, float ae_in, int32_t serial, uint32_t *state_out);
/* ---- TemporalBlendWithClamp (csrc/ycge_resident.cpp, kernels csrc/ycge_kernels.hip) on caller-given planes of w x h pixels: current / normal /
 * hist_in / prev_normal 3 f32 a pixel, depth / prev_depth f32, sky / prev_sky u8 holding 0 or 1; taa_alpha, taa_clamp_radius, taa_luminance_pad the
 * raw config values (TaaParams is derived as for a frame); reset != 0 the history restart.  form: 0 k_taa with guide outputs of their own, 1 the
 * guide inputs are the outputs, 2 no guide outputs (normal_out / depth_out / sky_out: the given normal / depth / sky as the device holds them),
 * 3 form 0 in the one-wavefront workgroups of frames in flight, 4 k_scatter_halo + k_taa_tiles, 5 k_resolve_tiles.  Forms 0-3: any w x h, a
 * one-device context, slab_out unused (may be NULL).  Forms 4-5: the context's own hiW x hiH as its rank of world_size, taa_clamp_radius <= 1;
 * the halo records are gathered from the caller's full frame over this rank's receive list, then every pixel of another rank is poisoned in
 * the planes TAA reads; outputs hold the inputs wherever this rank owns nothing; slab_out: the bytes of a history slab, zeros where no pixel is.
 * Buffers of its own: the context's history, guides, planes, taa_valid and committed camera are untouched, and so is what an existing ring
 * of the tile-resident form holds - but forms 4-5 CREATE that ring and the halo lists on a context that has none yet, as its first
 * tile-resident call would (a device synchronise, the ring's allocations, cleared cost and schedule words).  Refused:
 * frames in flight, a peer or multi-device context, and for forms 0-3 a rank of several */
int ycge_test_taa(ycge_ctx *c, int32_t form, int32_t reset, int32_t w, int32_t h, const float *current, const float *normal, const float *depth,
                  const uint8_t *sky, const float *hist_in, const float *prev_normal, const float *prev_depth, const uint8_t *prev_sky, float taa_alpha,
                  int32_t taa_clamp_radius, float taa_luminance_pad, float *hist_out, float *normal_out, float *depth_out, uint8_t *sky_out,
                  float *slab_out);

/* ---- the camera physics' stepper (csrc/ycge_camera_physics.h) on the host over a caller's Scene.Hit, no context and no device: the
 * arguments, refusals, caps and results of ycge_volume_camera_tick.  hit answers one ray {o xyz, d xyz, tmin, tmax} (d as handed to
 * new Ray: the callback normalises) with a non-zero return and rec = {t, p xyz, n xyz} on a hit, 0 on a miss.  windowed = 0: the
 * reference's serial order, a ray at a time; != 0: the device's window-and-commit order, each window's rays asked before any is folded */
typedef int (*ycge_camera_hit_fn)(void *user, const float ray[8], float rec[7]);
int ycge_test_camera_tick_host(ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves, int32_t n_moves,
                               float delta_time_ms, int32_t run_update, ycge_camera_tick_info *info, ycge_camera_hit_fn hit, void *user,
                               int32_t windowed, char *msg, size_t msg_bytes);
/* the same for a batch: the arguments, refusals (the text in msg names the body and the move) and per-body results of ycge_volume_bodies_tick,
 * body after body over the caller's Scene.Hit; no context and no device */
int ycge_test_bodies_tick_host(ycge_camera_body *bodies, const ycge_body_shape *shapes, int32_t n, const ycge_camera_world *world,
                               const ycge_camera_move *moves, const int32_t *move_first, float delta_time_ms, int32_t run_update,
                               ycge_body_result *results, ycge_camera_tick_info *info, ycge_camera_hit_fn hit, void *user, int32_t windowed,
                               char *msg, size_t msg_bytes);

/* the sixel presenter (csrc/ycge_sixel.cpp; tests/test_gpu_sixel.py).  ycge_test_pixels: k_sixel_pixels alone on a caller's hi-res buffer
 * (2 fbH ss rows of fbW ss samples, 3 f32 each) under `exposure`, whatever the context's framebuffer is: out_rgba W*H RGBA8, out_index W*H
 * registers, either may be NULL.  ycge_test_sixel_stream: the encoder's kernels alone on a caller's register plane of any W x H whose bound
 * fits; a value of 216 or more is refused on the host.  Neither touches frame, sixel or delta state */
int ycge_test_pixels(ycge_ctx *c, const float *hdr, int32_t fbW, int32_t fbH, int32_t ss, float exposure, int32_t dither, uint8_t *out_rgba, uint8_t *out_index);
int ycge_test_sixel_stream(ycge_ctx *c, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity,
                           size_t *out_len);
/* ycge_test_video_pixels: k_video_pixels alone on a caller's source frame and geometry, whatever the context's framebuffer is: out_rgba and
 * out_index of fbW ss x 2 fbH ss pixels, either may be NULL.  ycge_test_sixel_delta_stream: the delta encoder's kernels alone on two caller's
 * register planes (prev: what the terminal shows); out_info 4 words or NULL.  Both use buffers of their own and touch no context state */
int ycge_test_video_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t fbW, int32_t fbH, int32_t ss,
                           int32_t dither, uint8_t *out_rgba, uint8_t *out_index);
int ycge_test_sixel_delta_stream(ycge_ctx *c, const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out,
                                 size_t capacity, size_t *out_len, uint32_t *out_info);
/* the adaptive palette (csrc/ycge_sixel_palette.hip; tests/test_gpu_sixel_palette.py).  ycge_test_sixel_palette: the palette stage alone on a
 * caller's RGBA8 plane of any W x H <= 2^24 pixels: out_index W*H registers, out_palette 256 x RGBA8, out_pct 256 x 3, out_count, any of them
 * NULL.  ycge_test_sixel_palette_stream: the stage and the 256-register encoder's kernels.  Planes and encoder buffers of their own, no frame
 * or delta state - but `hold` reads the context's kept palette and a success replaces it, as the _palette calls do */
int ycge_test_sixel_palette(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t hold, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct,
                            int32_t *out_count);
int ycge_test_sixel_palette_stream(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, int32_t hold, uint8_t *out,
                                   size_t capacity, size_t *out_len);

/* ---- read-outs for tests and profiles (a context, a destination, a capacity; YCGE_OK or an error code) */
int ycge_debug_scene_bvh_stats(ycge_ctx *c, int64_t *out6);          /* how ycge_scene_update_objects built the tree: device / fallback / host builds, us, sort fallbacks, depth */
int ycge_debug_device_bvh(const float *bounds, const float *centroids, int32_t n, void *nodes_out, int32_t *leaf_out, uint32_t *result_out, void *build_out);   /* k_scene_bvh_build alone */
int ycge_debug_mesh_bvh_stats(ycge_ctx *c, int64_t *out8);           /* how ycge_scene_upload built the mesh BVHs: device builds, host builds, host builds after the device builder declined, us of the last device build; of the last upload: Array.Sort cases, deepest tree, wide nodes, subtree workgroups.  c = NULL: YCGE_ERR_INVALID_ARG and out8[0..2] = YCGE_MESH_BVH_HOST, _DEVICE_MIN, _WIDE_MIN as parsed now (no device) */
int ycge_debug_device_mesh_bvh(const float *tris9, int32_t n, void *nodes_out, int32_t *leaf_out, uint32_t *res16);   /* the device-side mesh BVH builder alone (csrc/ycge_mesh_bvh_build.hip), no context; what it declines the host builds.  res16: depth, Array.Sort cases, wide nodes, subtree workgroups, fallback reason (0: built on the device), built on the device, wide levels, us.  Returns the node count; YCGE_ERR_NO_DEVICE_CODE without a device */
int ycge_debug_device_mesh_arena(const float *tris9, int32_t n, void *out, int64_t capacity_bytes, uint32_t *root_ref_out, uint32_t *tl_offset_out, uint32_t *res8);   /* the twin of ycge_host_mesh_arena_treelets on the device, no context: the tree (device builder, or the host's tree uploaded when it declines), then records and treelets by csrc/ycge_mesh_emit.hip.  res8: tree built on the device, nodes, record units, us of layout / records / treelets, 0, 0.  Returns the arena's bytes; YCGE_ERR_NO_DEVICE_CODE without a device */
int ycge_debug_read_mesh_arena(ycge_ctx *c, void *dst, int64_t capacity_bytes, uint32_t *tl_offset_out);   /* the context's resident mesh arena (records, then the treelet region at *tl_offset_out, 0 = none), whichever side wrote it; returns its bytes */
int ycge_debug_read_meshes(ycge_ctx *c, void *dst, int32_t capacity_meshes);   /* the GMesh records the device holds (32 bytes each: root box, root reference); returns how many */
int ycge_debug_mesh_emit_stats(ycge_ctx *c, int64_t *out4);          /* who wrote the arena of the last upload: meshes emitted on the device, on the host, us of the last device layout + records + treelets, arena bytes.  c = NULL: YCGE_ERR_INVALID_ARG and out4[0..1] = YCGE_MESH_EMIT_HOST, _DEVICE_MIN as parsed now (no device) */
int ycge_debug_read_walk_tree(ycge_ctx *c, void *gnodes_out, void *walk_out, int32_t capacity_nodes, int32_t *grid_owner_out, int32_t n_grids, uint32_t *root_and_limit_out);
int ycge_debug_read_grid(ycge_ctx *c, int32_t grid_index, void *record_out /* sizeof GGrid = 112 bytes */, int32_t *materials_out);   /* a resident grid as the device holds it: its record and, per voxel in ycge_grid.cells order, the material of its cell code (-1 = empty) */
ycge_ctx *ycge_debug_peer_context(ycge_ctx *c, int32_t k);           /* the context of device k + 1 of a one-process multi-device context (NULL: none): the scene calls refuse it */
int ycge_debug_grid_pool_stats(ycge_ctx *c, int64_t *out12);         /* resident grids, free indices, arena bytes in use, arena capacity, arena growths, slots reused, device encodes, host-fallback encodes; the last attach in us: staging copy, host-to-device copy, encode kernel, read-back */
int ycge_debug_mesh_pool_stats(ycge_ctx *c, int64_t *out12);         /* the resident meshes (csrc/ycge_mesh_pool.cpp): resident meshes, free indices, units of records in use, capacity in units (before the first attach: the uploaded records), growths of the pooled arena, ranges reused, device builds, host builds of the attaches; the last attach in us: trees, emit, copies (re-homing, growth, other devices); 1 once the arena is pooled */
int ycge_debug_mesh_ranges(int64_t end0, int32_t n_index0, const int64_t *ops, int32_t n_ops, int64_t *out /* 4 per op */);   /* the pool's allocator alone (csrc/ycge_mesh_pool.h), no context and no device, from end0 units of records and n_index0 indices: n_ops triples {op, a, b} - 0 take a units, 1 give back the b units at unit a, 2 take an index, 3 give back index a; per op {the take's answer, the records' end, free ranges, free units} */
/* chunk generation, host only (csrc/ycge_worldgen.cpp over csrc/ycge_worldgen.h; tests/test_worldgen_hooks_cpu.py against tests/worldgen_restatement.py) */
int ycge_host_worldgen_noise(int32_t n, const int32_t *ix, const int32_t *iz, const float *x, const float *z, int32_t seed, uint32_t *hash_out, float *noise_out);   /* FastHash(ix, 0, iz, seed) and GradientNoise2D(x, z, seed) */
int ycge_host_worldgen_height(const ycge_world *world, int32_t n, const int32_t *gx, const int32_t *gz, int32_t *height_out);                                      /* TerrainNoise.HeightY */
int ycge_host_worldgen_river(const int32_t *tile /* (size + 2)^2 */, int32_t size, int32_t sea, int32_t *dir_out, float *accum_out, int32_t *carved_out, int32_t *river_water_out);   /* RiverNetwork.ComputeForChunk on a caller's height tile: D8 code (dx + 1) * 3 + (dz + 1), accum, carved ground, river surface */
int ycge_host_worldgen_carve(float accum, int32_t ground, int32_t sea, int32_t *carved_out, int32_t *river_water_out);                                               /* the carve and river-surface formulas at a given accumulation */
/* the pregenerated world, host only (tests/test_worldpregen_cpu.py against tests/worldpregen_restatement.py).  world_fields: the 2-D fields of a window as
 * ycge_worldgen_world_cells computes them, each nx * nz in x * nz + z order, NULL = skipped: ground before and after the river pass, D8 code, accum, slope, biome,
 * localWater, feature descriptor (csrc/ycge_worldgen.h), BiomeMap's dryness verdict alone (Forest / Desert whatever the height), StrataMap's noise verdict.
 * world_from_fields: the voxel fill and PlaceTreesGlobal on CALLER-GIVEN fields of nx x nz columns (feature NULL: the descriptors are made from the fields, origin (0, 0)) - gather = 0 the serial loops, != 0 the kernels' scheme on the
 * host (anyLeaves flags to a fixed point, then one gather per cell); *passes_out = 0 or the gather's passes */
int ycge_host_worldgen_world_fields(const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t *ground0_out,
                                    int32_t *ground_out, int32_t *dir_out, float *accum_out, float *slope_out, int32_t *biome_out, int32_t *water_out,
                                    uint32_t *feature_out, int32_t *climate_out, int32_t *rock_out);
int ycge_host_worldgen_river_global(const int32_t *ground /* nx * nz */, int32_t nx, int32_t nz, int32_t sea, int32_t *dir_out, float *accum_out, int32_t *carved_out,
                                    int32_t *river_water_out);       /* RiverNetworkGlobal.Compute on a caller's heights: D8 code, accum (the in-degree), carved ground, river surface */
int ycge_host_worldgen_world_from_fields(const ycge_world *world, int32_t nx, int32_t nz, const int32_t *ground, const int32_t *water, const float *slope,
                                         const int32_t *biome, const int32_t *rock, const uint32_t *feature, int32_t gather, int32_t *cells_out, int32_t *passes_out);
int ycge_debug_worldpregen_stats(ycge_ctx *c, int64_t *out5);        /* the last call of ycge_scene_generate_world, on the root device: anyLeaves passes (the last flips nothing); us of the 2-D field kernels, of the anyLeaves pass loop (wall time: a launch, a stream synchronise and a 4-byte read-back per pass), of the occupancy kernel and its read-back, of the fill kernels */
int ycge_debug_worldgen_stats(ycge_ctx *c, int64_t *out4);           /* ycge_scene_generate_grids: chunks made on the device, chunks made on the host, the last call's column kernel and fill + tree kernels in us (root device) */
int ycge_debug_obj_stats(ycge_ctx *c, int64_t *out6);               /* ycge_obj_parse: files the kernels parsed, files the host parser took, why the last one went to the host (0: it did not; 1 a float token outside the exact domain, 2 a line over the cap, 4 YCGE_OBJ_HOST, 8 below YCGE_OBJ_DEVICE_MIN), then wall us of the last parse's line marking + line walk + scans, of its token parsing + used / range / bounds pass, and of the last ycge_obj_triangles' pass.  c = NULL: YCGE_ERR_INVALID_ARG and out6[0..4] = the mark kernel's tile in bytes, the lines a workgroup of the line kernels takes, the line cap in bytes, YCGE_OBJ_DEVICE_MIN and YCGE_OBJ_HOST as parsed now (no device) */
int ycge_debug_obj_ground_stats(ycge_ctx *c, int64_t *out6);        /* ycge_obj_ground: tails the kernels ran, tails the host ran, why the last one went to the host (0: it did not; 1 a walk or a hook passed its bound of n_positions steps, 2 the round cap, 4 YCGE_OBJ_GROUND_HOST, 8 below YCGE_OBJ_GROUND_DEVICE_MIN), the labelling rounds of the last device tail (hook + flatten launches; the last one hooks nothing: 2 on a clean run), the sums of the last tail that fell back to a serial path (0: no chunked sum is built, every sum is the serial chain), wall us of the last tail.  c = NULL: YCGE_ERR_INVALID_ARG and out6[0..4] = the terms one trip of the sum takes, the round cap, YCGE_OBJ_GROUND_DEVICE_MIN_DEFAULT, YCGE_OBJ_GROUND_DEVICE_MIN and YCGE_OBJ_GROUND_HOST as parsed now (no device) */
int ycge_debug_obj_ground_phases(ycge_ctx *c, int64_t *out5);       /* contexts made with YCGE_OBJ_GROUND_PHASES (a stream synchronise behind every phase): wall us of the last device tail's labelling rounds, count + winner, terms, the three sums, bounds + read-back; zeros otherwise */
int ycge_debug_world_store_chunk(ycge_ctx *c, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t dims_out[3]);   /* the raw cells of one chunk of the world store as k_ws_slice writes them (a host store: as the host loop does), ycge_grid.cells order, and its clipped sizes; runs no attach.  cells_out = NULL: the sizes alone.  YCGE_ERR_INVALID_ARG: no store, no such chunk */
int ycge_debug_world_store_stats(ycge_ctx *c, int64_t *out8);       /* the world store: the bytes it actually holds (0: none; a fields store: its 2-D fields), the slabs of the last load, us of that load's copies into the staging (wall), its host-to-device copies and its occupancy kernels (stream time, root device: they overlap each other), us of the last ycge_scene_attach_world_chunks' slice kernels (root device), chunks sliced on the device and on the host since the context was made */
int ycge_debug_world_store_generate_stats(ycge_ctx *c, int64_t *out9);       /* the last ycge_world_store_generate on the root device: the form asked for (-1: none yet), 1 when the host generator made the cells (YCGE_WORLDGEN_HOST / YCGE_WORLD_STORE_HOST), the anyLeaves passes (the last flips nothing), the slabs of k_wp_planes (CELLS form), then us: the 2-D field kernels, the anyLeaves pass loop (WALL time: each pass is a launch, a stream synchronise and a 4-byte read-back), the occupancy kernel and its read-back, the k_wp_planes and k_ws_occupied launches (stream time), the host generator */
int ycge_debug_read_post_progress(ycge_ctx *c, uint32_t *dst, size_t n_words);               /* k_atrous_stream's per-band records (profiles/post_bands.py) */
int ycge_debug_read_wave_prof(ycge_ctx *c, unsigned long long *dst, size_t n_u64);            /* per-wavefront begin / end / steps of a profiling build (profiles/mega_prof.py) */
int ycge_debug_read_coop_stats(ycge_ctx *c, uint64_t out[16]);                               /* -DYCGE_DBG_COOPSTAT builds */
int ycge_debug_read_batch_stats(ycge_ctx *c, uint64_t out[64]);
int ycge_debug_resident_loop(ycge_ctx *c, int32_t frames, double *period_ms, double *issue_ms);   /* a rank's tile-resident ring driven from C (profiles/rank_times.py) */
int ycge_debug_live_resources(int64_t out[6]);                       /* process-wide, no context and no device needed: {device allocations, device bytes, events, streams, page-locked allocations, page-locked bytes} the library holds right now (csrc/ycge_own.h) */
int ycge_debug_is_page_locked(const void *p, size_t bytes);          /* the verdict ycge_render_frame takes on a caller's SDR buffer: 1 page-locked over its whole range */
int ycge_debug_throw(ycge_ctx *c, int32_t kind);                     /* throws INSIDE an export (1 std::bad_alloc, 2 std::runtime_error, 3 an int, 4 std::length_error, 5 std::system_error; 0 nothing): the exception barrier's test */
int ycge_debug_fail_allocation(int64_t nth);                         /* lib/var_faultinject.so ONLY (-DYCGE_FAULT_INJECTION): the library's n-th allocation from now throws std::bad_alloc */

/* ---- host translation units -> kernel translation units (sizes and knobs of what the .hip files define) */
size_t ycge_wf_sizes(int which);
size_t ycge_post_state_bytes(void);
size_t ycge_exposure_scratch_bytes(int w, int h, int step);
size_t ycge_bvh_build_scratch_bytes(int n);
size_t ycge_mesh_bvh_sizes(int which);
int ycge_atrous_persist_resident(int groups_per_pass, int split, int profile);
void ycge_atrous_duo_pad_lds(int bytes);
void ycge_peer_worker_main(ycge_ctx *c, ycge_ctx *p);                /* a peer device's thread function (started by ycge_create) */

#ifdef __cplusplus
}
#endif
#endif
