/*
 * ycge.h — C-ABI of the MI355X ray-trace core for YetAnotherConsoleGameEngine.
 *
 * This is the drop-in boundary for ONE path of the reference: the per-pixel
 * ray-trace loop that RaytraceEntity drives through the private seam
 * RaytraceEntity.IConsoleRenderer (reference ConsoleGame/RaytraceEntity.cs:12-18:
 * SetCamera / SetFov / TryFlipAndBlit / Resize).  A third IConsoleRenderer
 * wrapper on the C# side P/Invokes the entry points below (binding source in
 * INTEGRATION.md).  Everything is plain C: PODs, pointers and sizes; no C++
 * or torch types cross this line.
 *
 * Conventions
 *   - every function returns YCGE_OK (0) or a negative ycge_status; nothing
 *     throws across the ABI (the reference throws on misuse, e.g.
 *     Scenes/Scene.cs:73; the C# wrapper turns codes back into exceptions);
 *   - the caller owns every host pointer it passes; the library copies during
 *     the call; the context owns all device memory;
 *   - calls on one context come from one thread (reference: the Terminal loop
 *     thread, Renderer/Terminal.cs:136-176) except ycge_set_camera, which is
 *     safe against a concurrent ycge_render_frame (reference lock(camLock),
 *     RayTracing/RaytraceRenderer.cs:142-147).
 *
 * All float data is IEEE binary32, little endian.  "hi-res grid" below is the
 * reference's trace grid hiW = fbW*ss, hiH = fbH*2*ss
 * (RayTracing/RaytraceRenderer.cs:83-87); per-pixel buffers are row-major,
 * index = x + y*hiW (RayTracing/Fast2D.cs:21-24).
 */
#ifndef YCGE_H
#define YCGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YCGE_ABI_VERSION 10
#define YCGE_MAX_DEVICES 8

typedef enum ycge_status {
    YCGE_OK = 0,
    YCGE_ERR_INVALID_ARG = -1,   /* null pointer, bad size, bad enum            */
    YCGE_ERR_NO_SCENE = -2,      /* render before scene upload (Scene.cs:73)    */
    YCGE_ERR_DEVICE = -3,        /* HIP runtime error; see ycge_last_error      */
    YCGE_ERR_UNSUPPORTED = -4,   /* feature outside the path (textures, ...)    */
    YCGE_ERR_OUT_OF_MEMORY = -5,
    YCGE_ERR_STACK_DEPTH = -6,   /* BVH deeper than the reference's fixed stacks
                                    (BVH.cs:118 = 128, MeshBVH.cs:150 = 64)     */
    YCGE_ERR_NO_DEVICE_CODE = -7,/* HIP kernels missing / no gfx950 device      */
    YCGE_ERR_INTERNAL = -8       /* a C++ exception other than std::bad_alloc (which is
                                    YCGE_ERR_OUT_OF_MEMORY) was stopped at the boundary:
                                    every export is a function-try-block, nothing unwinds
                                    into the caller (csrc/ycge_ctx.h: abi_catch)        */
} ycge_status;

typedef struct ycge_vec3 { float x, y, z; } ycge_vec3;

/* ---------------------------------------------------------------- materials
 * The reference passes opaque delegates Func<Vec3,Vec3,float,Material>
 * (Objects/Surfaces.cs:64) / Func<int,int,Material> (Objects/VolumeGrid.cs:189).
 * Only three shapes occur in its scene builders (Scenes/Scenes.cs:408-428,
 * Scenes/VoxelMaterialPalette.cs:29-98): constant, emissive constant, checker.
 * Material doubles (Material.cs:7-18) are narrowed to float here; the tracer
 * only ever reads them through (float) casts or compares against 0.0.
 */
typedef enum ycge_material_kind {
    YCGE_MAT_CONSTANT = 0,       /* Solid / Emissive / plain Material struct    */
    YCGE_MAT_CHECKER = 1,        /* Scenes.cs:418-428: parity of floor(x/s)+floor(z/s) */
    YCGE_MAT_TEXTURED = 2        /* a constant Material with DiffuseTexture != null: SampleAlbedo blends the albedo with a
                                    bilinear sample of the texture at the hit's (U, V) (RaytraceRenderer.cs:724-735 ->
                                    Renderer/Texture.cs:142-163 for a static texture, Texture.cs:113-140 for a LIVE one - camera /
                                    video frames, see ycge_texture.frame_bytes_per_pixel and ycge_scene_update_texture) */
} ycge_material_kind;

/* Renderer/Texture.cs:15,22-23: `pixels[y * width + x]` as RGBA32.ToInt() packs them (RGBA32.cs:14-31: byte 0 = r,
 * 1 = g, 2 = b, 3 = a of the little-endian int). */
typedef struct ycge_texture {
    int32_t width, height;       /* both >= 1                                   */
    const uint32_t *pixels;      /* width * height (static textures)            */
    /* A LIVE texture (`new Texture(IFrameReader, useRGBA, flipU, flipV)`, Renderer/Texture.cs:51-66: camera / video frames): bytes per
     * pixel of the frames, 3 = BGR or 4 = BGRA (dynamicBytesPerPixel); 0 = a static texture.  SampleBilinear then takes its other
     * branch (Texture.cs:113-140: flips, neighbours CLAMPED at the last row / column, bytes in B, G, R order, no per-lerp Saturate). */
    int32_t frame_bytes_per_pixel;
    int32_t flip_u, flip_v;
    /* the frame GetCurrentFramePtr() shows at upload: width * height * frame_bytes_per_pixel bytes (NULL: black until the first
     * ycge_scene_update_texture).  `pixels` is not read for a live texture. */
    const uint8_t *frame;
} ycge_texture;

typedef struct ycge_material {
    int32_t kind;                /* ycge_material_kind                          */
    ycge_vec3 albedo;            /* constant albedo, or checker colour A        */
    ycge_vec3 albedo_b;          /* checker colour B                            */
    float checker_scale;
    float specular;              /* carried for symmetry; never read (quirk 2)  */
    float reflectivity;
    ycge_vec3 emission;
    float transparency;
    float index_of_refraction;
    ycge_vec3 transmission_color;
    /* YCGE_MAT_TEXTURED only (Material.cs:16-18; doubles as in the reference: SampleAlbedo compares and clamps them as
     * doubles before it narrows) */
    int32_t texture;             /* index into ycge_scene.textures              */
    int32_t reserved;
    double texture_weight;       /* Material.TextureWeight; <= 0 means no texture */
    double uv_scale;             /* Material.UVScale                            */
} ycge_material;

/* --------------------------------------------------------------- primitives
 * One record per entry of Scene.Objects, in Objects order (order is part of
 * the result: BVH leaf order and tie-breaking depend on it).
 */
typedef enum ycge_prim_type {
    YCGE_PRIM_SPHERE = 0,        /* p = cx,cy,cz,radius              BoundedObjects.cs:7-69   */
    YCGE_PRIM_PLANE = 1,         /* p = px,py,pz, nx,ny,nz (n as given; normalised inside) Surfaces.cs:8-71 */
    YCGE_PRIM_DISK = 2,          /* p = cx,cy,cz, nx,ny,nz, radius   Surfaces.cs:73-142       */
    YCGE_PRIM_XYRECT = 3,        /* p = x0,x1,y0,y1,z                Surfaces.cs:144-214      */
    YCGE_PRIM_XZRECT = 4,        /* p = x0,x1,z0,z1,y                Surfaces.cs:216-286      */
    YCGE_PRIM_YZRECT = 5,        /* p = y0,y1,z0,z1,x                Surfaces.cs:288-358      */
    YCGE_PRIM_BOX = 6,           /* p = min xyz, max xyz             BoundedObjects.cs:72-116 */
    YCGE_PRIM_CYLINDER_Y = 7,    /* p = cx,cy,cz,radius,yMin,yMax,capped(0/1) BoundedObjects.cs:118-247 */
    YCGE_PRIM_TRIANGLE = 8,      /* p = A xyz, B xyz, C xyz          Objects/Triangle.cs      */
    YCGE_PRIM_MESH = 9,          /* ref = index into ycge_scene.meshes                        */
    YCGE_PRIM_VOLUME_GRID = 10   /* ref = index into ycge_scene.grids                         */
} ycge_prim_type;

typedef struct ycge_prim {
    int32_t type;                /* ycge_prim_type                              */
    int32_t material;            /* index into ycge_scene.materials (unused for mesh / grid) */
    int32_t ref;                 /* mesh / grid index                           */
    int32_t reserved;
    float p[12];
    /* Plane / Disk / Rects / Box overwrite the material func's Specular and
     * Reflectivity with their ctor arguments (Surfaces.cs:65-66,136-137,
     * 208-209,280-281,352-353).  Ignored for the other types. */
    float specular;
    float reflectivity;
} ycge_prim;

/* Triangle soup of one Mesh (RayTracing/Mesh.cs:16-21): 9 floats per triangle
 * (A, B, C), already transformed as MeshLoader.FromObj leaves them. */
typedef struct ycge_mesh {
    const float *triangles;      /* 9 * n_triangles floats                      */
    int32_t n_triangles;
    int32_t material;            /* material of every triangle                  */
    const int32_t *tri_material; /* optional per-triangle material, or NULL     */
} ycge_mesh;

/* (matId, metaId) -> material; stands in for Func<int,int,Material>. */
typedef struct ycge_voxel_lookup {
    int32_t mat_id;
    int32_t meta_id;
    int32_t material;            /* index into ycge_scene.materials             */
} ycge_voxel_lookup;

/* One VolumeGrid (Objects/VolumeGrid.cs:55-93).  cells = the ctor's
 * (int,int)[nx,ny,nz] in its native memory order: pair index
 * (ix*ny + iy)*nz + iz, Item1 = matId, Item2 = metaId.
 * Limits (YCGE_ERR_UNSUPPORTED beyond them): fewer than 2^30 cells per grid,
 * fewer than 2^23 8x8x8 bricks across any face, at most 255 distinct
 * (matId, metaId) pairs per grid, 4 GiB of voxel bytes per scene. */
typedef struct ycge_grid {
    int32_t nx, ny, nz;
    ycge_vec3 min_corner;
    ycge_vec3 voxel_size;
    const int32_t *cells;        /* 2 * nx*ny*nz int32                          */
    const ycge_voxel_lookup *lookup;
    int32_t n_lookup;
    int32_t default_material;    /* lookup miss -> this material; <0 = error    */
    int32_t wireframe;           /* ctor default true                           */
    float wire_width_fraction;   /* ctor default 0.06f                          */
    float wire_max_distance;     /* ctor default 16.0f                          */
} ycge_grid;

typedef struct ycge_light {      /* Objects/PointLight.cs:3-15 */
    ycge_vec3 position;
    ycge_vec3 color;
    float intensity;
} ycge_light;

typedef struct ycge_scene {      /* Scenes/Scene.cs:12-24 */
    const ycge_material *materials; int32_t n_materials;
    const ycge_prim *prims;         int32_t n_prims;
    const ycge_mesh *meshes;        int32_t n_meshes;
    const ycge_grid *grids;         int32_t n_grids;
    const ycge_light *lights;       int32_t n_lights;
    ycge_vec3 ambient_color;  float ambient_intensity;
    ycge_vec3 background_top;
    ycge_vec3 background_bottom;
    int32_t is_volume_scene;     /* `scene is VolumeScene` (RaytraceRenderer.cs:761) */
    int32_t n_textures;
    const ycge_texture *textures;   /* what YCGE_MAT_TEXTURED materials index */
    /* Scene.HasDynamicTextures (Scenes/Scene.cs:30): the host rewrites texture pixels between frames (video, camera), so
     * every frame (re)initialises the TAA history - `resetHistory = ... || scene.HasDynamicTextures`, RaytraceRenderer.cs:171. */
    int32_t has_dynamic_textures;
} ycge_scene;

/* ------------------------------------------------------------------- config */
typedef struct ycge_config {
    int32_t abi_version;         /* YCGE_ABI_VERSION                            */
    int32_t fb_width;            /* chexel columns  (Framebuffer.Width)         */
    int32_t fb_height;           /* chexel rows     (Framebuffer.Height)        */
    int32_t super_sample;        /* ss >= 1                                     */
    float fov_deg;
    int32_t device;              /* HIP device ordinal                          */
    /* framebuffer tiling across GPUs: this context traces the 32x8-pixel
     * tiles with tile_id % world_size == rank (one process per GPU). */
    int32_t rank;
    int32_t world_size;
    /* constants of RaytraceRenderer.cs:31-43,65,218 (same defaults) */
    int32_t diffuse_bounces;     /* 1 */
    int32_t max_mirror_bounces;  /* 2 */
    int32_t max_refractions;     /* 2 */
    float mirror_threshold;      /* 0.9f */
    float eps;                   /* 1e-4f */
    uint64_t seed_salt;          /* 0x9E3779B97F4A7C15 */
    float taa_alpha;             /* 0.01f */
    float motion_trans_reset;    /* 0.0025f */
    float motion_rot_reset;      /* 0.0025f */
    float diffuse_sigma_deg;     /* 25.0f */
    int32_t taa_clamp_radius;    /* 1 */
    float taa_luminance_pad;     /* 0.10f */
    /* denoise / tonemap stage after TAA (RaytraceRenderer.cs:221-227) */
    int32_t atrous_iterations;   /* 3 */
    float atrous_c_phi, atrous_n_phi, atrous_z_phi, atrous_a_phi; /* 3, 0.35, 2, 0.20 */
    int32_t capture_debug;       /* also keep rays / primId / hitT buffers      */
    int32_t count_work;          /* keep per-frame traversal counters           */
    /* tiled frame (world_size > 1): 1 = slabs carry the albedo plane (11 floats
     * per pixel; the denoise stage needs it), 0 = lean slabs of 8 floats per
     * pixel (hdr, normal, depth, sky: what TAA needs) - 27 % less all-gather
     * traffic; ycge_resolve_gathered then refuses an SDR buffer. Default 1.  */
    int32_t slab_albedo;
    /* One process, several GPUs (the reference makes ONE TryFlipAndBlit call from one process,
     * RaytraceEntity.cs:230): n_devices >= 2 makes ycge_render_frame drive devices[0 .. n_devices) itself -
     * tiles dealt round-robin over them, every device traces its share, the peers write their tiles straight
     * into devices[0]'s frame buffers over xGMI (no staging slabs), TAA and the post stage run on devices[0].
     * rank / world_size must then be 0 / 1.  n_devices 0 or 1 = the single GPU `device`. */
    int32_t n_devices;
    int32_t devices[YCGE_MAX_DEVICES];
    /* ApplyAtrousDenoise's buffer swap (RaytraceRenderer.cs:718) makes iteration 1 run IN PLACE - scan-order dependent, a dependent chain of
     * W/2 + 3H/2 pixel levels that costs 1.9 ms of a 1080p frame (8.8 ms at 3840x2160) however it is scheduled.  1 (default) reproduces it
     * bit for bit.  0 WAIVES it (SURVEY 8-f1 allows "reproduce or explicitly waive"): iteration 1 reads A and writes B like any other
     * iteration - the denoiser the C# text reads like, fully parallel (~0.2 ms).  The two differ by what INTEGRATION.md states (a filter
     * tap that sees a neighbour's already-filtered value instead of its unfiltered one); everything up to TAA is unaffected. */
    int32_t atrous_inplace_exact;
    /* tile-resident form (ycge_trace_tiles_resident): frame sets in the ring = tiled traces that may be in flight at a time, 2..15; 0 = 2 */
    int32_t tile_ring;
    /* One process, several GPUs (n_devices >= 1): how the devices' tiles come together on devices[0] (ABI 9).
     * YCGE_EXCHANGE_PEER_PUSH (0, default): the peers write their tiles straight into devices[0]'s frame buffers (k_push_tiles, no collective).
     * YCGE_EXCHANGE_RCCL (1): every device packs its tiles into a slab, ONE ncclAllGather over the devices' in-process communicators
     * (ncclCommInitAll; librccl.so is dlopen'ed, the library does not link it) reassembles the frame, devices[0] un-permutes it and runs
     * TAA and the post stage - the all-gather of SURVEY 8(e) behind the one TryFlipAndBlit call a single-process host makes.  Same pixels.
     * Where librccl.so or its symbols are missing the context falls back to the peer push; ycge_exchange_query says which is in use.
     * n_devices = 1 with YCGE_EXCHANGE_RCCL is a world of one (the frame goes through slab, all-gather and un-permute): what a one-GPU
     * box can test.  RCCL refuses two ranks on one device: devices[] must then be distinct. */
    int32_t multi_device_exchange;
} ycge_config;

typedef enum ycge_exchange { YCGE_EXCHANGE_PEER_PUSH = 0, YCGE_EXCHANGE_RCCL = 1 } ycge_exchange;

typedef struct ycge_frame_stats {
    int64_t frame;               /* frameCounter after the increment            */
    int32_t history_reset;       /* TAA history was (re)initialised this frame  */
    int32_t fan_blocks;          /* reserved, always 0 */
    double trace_ms;             /* device time of ray-gen + trace              */
    double taa_ms;
    double post_ms;              /* denoise + exposure + tonemap/downsample     */
    double total_ms;             /* wall time of the call                       */
    /* traversal counters; valid when config.count_work != 0 */
    uint64_t n_rays;             /* Scene.Hit + Scene.Occluded calls            */
    uint64_t n_box;              /* AABB evaluations as root or as child        */
    uint64_t n_tri;              /* MeshBVH.TriHit calls                        */
    uint64_t n_prim;             /* analytic primitive tests (box = 6 rects)    */
    uint64_t n_vox;              /* DDA cells visited                           */
    float exposure;              /* ToneMapper.EffectiveExposure                */
    float exposure_serial_chunks;/* diagnostics: 512-term chunks of the exposure sum that took the one-by-one path */
    /* of n_rays: shadow queries towards lights of Intensity == 0 (counted with config.count_work).  The reference traces them although
     * their contribution is a zero whatever they find (RaytraceRenderer.cs:586-602); the timed kernels do not. */
    uint64_t n_rays_dark;
    /* tiles traced by each device of this frame (one entry for a single-GPU context; devices[] order) */
    int32_t n_devices_traced;
    int32_t device_tiles[YCGE_MAX_DEVICES];
} ycge_frame_stats;

typedef enum ycge_buffer {
    YCGE_BUF_RAYS = 0,           /* 6 f32/px: origin, dir      (capture_debug)  */
    YCGE_BUF_PRIM_ID = 1,        /* i32/px: Objects index of primary hit, -1 miss (capture_debug) */
    YCGE_BUF_SUB_ID = 2,         /* i32/px: triangle index / box face / voxel cell (capture_debug) */
    YCGE_BUF_HIT_T = 3,          /* f32/px: primary hit t, FLT_MAX miss (capture_debug) */
    YCGE_BUF_CURRENT_HDR = 4,    /* 3 f32/px */
    YCGE_BUF_G_ALBEDO = 5,       /* 3 f32/px */
    YCGE_BUF_G_NORMAL = 6,       /* 3 f32/px */
    YCGE_BUF_G_DEPTH = 7,        /* f32/px   */
    YCGE_BUF_SKY_MASK = 8,       /* u8/px    */
    YCGE_BUF_TAA_HISTORY = 9,    /* 3 f32/px */
    YCGE_BUF_PREV_NORMAL = 10,   /* 3 f32/px */
    YCGE_BUF_PREV_DEPTH = 11,    /* f32/px   */
    YCGE_BUF_PREV_SKY = 12,      /* u8/px    */
    YCGE_BUF_DENOISED = 13,      /* 3 f32/px */
    YCGE_BUF_RNG_STATE = 14      /* u64/px: Rng state when the pixel finished (capture_debug) */
} ycge_buffer;

/* flattened acceleration structures, for parity tests of the builders */
typedef enum ycge_accel {
    YCGE_ACCEL_SCENE_NODES = 0,  /* 10 x 4 B per node: min xyz, max xyz, left, right, start, count (BVH.cs:11-20) */
    YCGE_ACCEL_SCENE_LEAF_INDEX = 1, /* i32 leafObjIndex                        */
    YCGE_ACCEL_MESH_NODES = 2,   /* same node record, mesh `index`              */
    YCGE_ACCEL_MESH_LEAF_INDEX = 3   /* i32 leafTriIndex                        */
} ycge_accel;

typedef struct ycge_ctx ycge_ctx;

/* Fill *cfg with the reference defaults (RaytraceRenderer.cs:31-43,65,218-224). */
int ycge_config_default(ycge_config *cfg);

/* new RaytraceRenderer(fb, scene, fov, pxW, pxH, ss)   RaytraceEntity.cs:97,240,262 */
int ycge_create(const ycge_config *cfg, ycge_ctx **out);
/* dispose */
void ycge_destroy(ycge_ctx *ctx);
/* message of the last failing call on ctx (or of ycge_create when ctx == NULL) */
const char *ycge_last_error(const ycge_ctx *ctx);

/* scene.RebuildBVH()   RaytraceRenderer.cs:107, RaytraceEntity.cs:244, Scene.cs:122-127.
 * Builds the scene BVH (Objects/BVH.cs:258-459) and every mesh BVH
 * (Objects/MeshBVH.cs:371-576) and uploads them.  A mesh BVH is built
 * bit-faithfully, on the device from N triangles on
 * (N = YCGE_MESH_BVH_DEVICE_MIN, default 4 000: the measured crossover,
 * profiles/mesh_build_rate.json) and on the host below. */
int ycge_scene_upload(ycge_ctx *ctx, const ycge_scene *scene);
/* per-frame entity animation of lights / sky (Scenes/DayNightCycle.cs:80-89) */
int ycge_scene_update_lights(ycge_ctx *ctx, const ycge_light *lights, int32_t n_lights,
                             const ycge_vec3 *ambient_color, float ambient_intensity,
                             const ycge_vec3 *background_top, const ycge_vec3 *background_bottom);

/* Scene.Update() -> RebuildBVH() after an entity moved its geometry (Scenes/Scene.cs:122-127; e.g.
 * BobbingSphereEntity.Update, Scenes/TestScenesRandom.cs:708-714): replaces the Scene.Objects records and
 * rebuilds the scene-level BVH only.  `prims` index the materials and meshes of the last ycge_scene_upload (a Mesh keeps its own
 * BVH in the reference too, Mesh.cs:14) and the RESIDENT grids: those of the upload and of ycge_scene_attach_grids, less the detached.
 * Likewise the RESIDENT meshes and the materials appended since (ycge_scene_attach_meshes, ycge_scene_append_materials below).  The tree (Objects/BVH.cs:258-459,
 * same nodes, numbering and leaf order) is built on the device for up to 2 560 objects - the host only flattens the
 * records and their boxes - and by the host builder above that. */
int ycge_scene_update_objects(ycge_ctx *ctx, const ycge_prim *prims, int32_t n_prims);

/* --- chunk streaming: VolumeScene.Update calls WorldManager.LoadChunksAround every frame (Scenes/VolumeScenes.cs:63-64): chunks that
 * entered the view are attached as new VolumeGrids, chunks that left are removed from Scene.Objects and cached (WorldManager.cs:289-370).
 * Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, ycge_config and ycge_scene are unchanged - a host detects these two
 * exports by symbol lookup.  One LoadChunksAround tick is: attach what entered, ycge_scene_update_objects with the new object list,
 * detach what left - or leave it resident and merely unreferenced, which is the reference's chunk cache (CacheChunk /
 * TryAttachFromCache).  Each of the three steps leaves a complete, renderable scene.
 *   Same pixels.  After any sequence of attach / update_objects / detach, every frame, every ycge_read_buffer buffer, every scene query,
 *     the counting instances' ycge_frame_stats counters and ycge_read_timed_steps are what the same context gives when each tick is
 *     instead one ycge_scene_upload of the equivalent scene (same materials, same Scene.Objects in the same order, the grids they refer
 *     to) - bit for bit, TAA history and exposure state included.  Grid indices, cell codes and arena offsets are internal and may differ.
 *   Indices.  A grid of the upload keeps its index.  An attached grid takes the lowest free index (slots are reused); out_grid_index is
 *     written only on success.  The next ycge_scene_upload forgets all of it.
 *   Limits are ycge_grid's own (2^30 cells, 2^23 bricks per face, 255 distinct pairs, 4 GiB of voxel bytes RESIDENT), refused with the
 *     statuses ycge_scene_upload gives.  n = 0 is YCGE_OK.  YCGE_ERR_NO_SCENE before the first upload.  A grid that is wrong in two
 *     ways - a pair with no material and more than 255 distinct pairs - is refused as the former (YCGE_ERR_INVALID_ARG, the message names
 *     the lowest such cell in `cells` order), where ycge_scene_upload reports whichever its walk meets first.
 *   All or nothing.  A refused or failed attach (bad argument, a pair with no material and default_material < 0, a limit, an allocation
 *     failure) leaves the scene exactly as it was - renderable, no slot taken, out_grid_index untouched.  Stronger than ycge_scene_upload
 *     (which leaves no scene) on purpose: a streaming host must survive one bad chunk.
 *   A scene uploaded with no grid may receive grids: the kernel instantiation, the walk tree and the stage-pipeline decision follow at the
 *     next ycge_scene_update_objects, as after an upload of the equivalent scene - they follow the grids Scene.Objects refer to, so
 *     grids that stay resident and unreferenced (the chunk cache) change nothing.
 *   Several devices: the devices of a one-process multi-device context are served one after the other (an attach is serial in their number).
 *   Frames in flight.  ycge_scene_attach_grids JOINS the frames in flight, like every other scene call: it may move the cell arena, the
 *     material tables and the grid table, which the frames read (ycge_scene_update_objects, the next step of a tick, joins them anyway).
 *     ycge_scene_detach_grids changes host state only and joins nothing.  Scene queries see the new grids with the next query.
 *   One-process multi-device (n_devices >= 2): the root forwards to its peers as ycge_scene_upload does; a peer context refuses.  Tiled
 *     ranks (world_size > 1) each make the same calls, like every other scene call.
 * The raw cells go up once through page-locked staging and are encoded on the device (csrc/ycge_grid_encode.hip); a grid whose lookup
 * table has more than 254 entries takes the host encoder of ycge_scene_upload. */
/* Make n more grids resident beside those of the last ycge_scene_upload.  No object refers to them yet: the next
 * ycge_scene_update_objects may (ycge_prim.ref = out_grid_index[k]).  Materials index the materials of the last upload. */
int ycge_scene_attach_grids(ycge_ctx *ctx, const ycge_grid *grids, int32_t n, int32_t *out_grid_index /* n */);
/* Give n grids' slots back.  Refused (YCGE_ERR_INVALID_ARG, nothing freed) while the current Scene.Objects refer to one of them,
 * for an index that is not resident, or for one named twice. */
int ycge_scene_detach_grids(ycge_ctx *ctx, const int32_t *grid_index, int32_t n);

/* --- meshes and materials of a resident scene: a host that adds one model to a running scene - a viewer that loads a second .obj, an entity
 * whose GetHittables() yields a Mesh (Scenes/Scene.cs:519-535) - attaches it, instead of paying for every mesh BVH, the whole arena and every
 * grid again with ycge_scene_upload.  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing struct changes - a host
 * detects these exports by symbol lookup.  One tick is: append the materials that are new, attach the meshes that are new,
 * ycge_scene_update_objects with the new object list, detach what left - or leave it resident and merely unreferenced.  Each step leaves a
 * complete, renderable scene.
 *   Same pixels.  After any sequence of append / attach / update_objects / detach, every frame, every ycge_read_buffer buffer, every scene
 *     query, the counting instances' ycge_frame_stats counters and ycge_read_timed_steps are what the same context gives when each tick is
 *     instead one ycge_scene_upload of the equivalent scene - bit for bit, TAA history and exposure state included.  The equivalent scene
 *     holds the same materials in the same order and the same Scene.Objects in the same order; its meshes[i] is the resident mesh of index
 *     i, a free index a mesh of 0 triangles.  Arena offsets are internal and may differ.
 *   Indices.  A mesh of the upload keeps its index.  An attached mesh takes the lowest free index; out_mesh_index is written only on
 *     success.  The next ycge_scene_upload forgets all of it.
 *   Referencing.  No object refers to an attached mesh until the next ycge_scene_update_objects names it (ycge_prim.ref).  A mesh that
 *     stays resident and unreferenced changes nothing.
 *   Materials.  A mesh's `material` and `tri_material` index the materials of the last upload plus everything appended since.
 *   All or nothing.  A refused or failed attach or append leaves the scene exactly as it was - renderable, no index taken, no range of the
 *     arena taken, the outputs untouched; every refusal is decided before the pool of resident meshes is changed.  YCGE_ERR_INVALID_ARG:
 *     n < 0, NULL arrays with n > 0, n_triangles < 0, NULL `triangles` with triangles, a material out of range, a peer context (the
 *     message names the mesh by its place in the call).  YCGE_ERR_NO_SCENE before the first upload.  A leaf of more than 15 triangles and a
 *     tree deeper than 64 are refused with the statuses and texts ycge_scene_upload gives.  YCGE_ERR_UNSUPPORTED when the records would pass
 *     what a pooled arena can address (the message gives the limit in bytes).  YCGE_ERR_OUT_OF_MEMORY for a failed allocation.  n = 0 is
 *     YCGE_OK.
 *   Frames in flight.  An attach and an append JOIN the frames in flight, like every other scene call: the arena and the tables may move.
 *     ycge_scene_detach_meshes changes host state only and joins nothing.  Scene queries see the change with the next query after
 *     ycge_scene_update_objects.  What the kernels are told about the resident SET - whether any resident mesh has an inner node, the
 *     deepest resident tree, the flags of the material list - follows it with the next ycge_scene_update_objects, as after an upload of
 *     the equivalent scene.
 *   One-process multi-device (n_devices >= 2): the root builds once and forwards - every other device receives the new records and
 *     treelets by a device copy; a peer context refuses.  Tiled ranks (world_size > 1) each make the same calls.
 * The trees are built as ycge_scene_upload builds them (the device builder from YCGE_MESH_BVH_DEVICE_MIN triangles on, the host builder
 * below that and for what the device builder declines); every mesh's records and treelets are written on the device (csrc/ycge_mesh_emit.hip). */
/* Make n more meshes resident beside those of the last ycge_scene_upload. */
int ycge_scene_attach_meshes(ycge_ctx *ctx, const ycge_mesh *meshes, int32_t n, int32_t *out_mesh_index /* n */);
/* Give n meshes' indices and records back.  Refused (YCGE_ERR_INVALID_ARG, nothing freed) while the current Scene.Objects refer to one of
 * them, for an index that is not resident, or for one named twice. */
int ycge_scene_detach_meshes(ycge_ctx *ctx, const int32_t *mesh_index, int32_t n);
/* n more materials behind the existing ones; *out_first_index is the first new index.  A textured material indexes the textures of the last
 * upload.  The flags derived from the material list (some material is transparent, textured, can mirror - and with that the rounds of the
 * wavefront path) follow the longer list and are published with the next install of the objects: an append alone changes no frame, and
 * from the tick's ycge_scene_update_objects on the equivalence above holds.  Grid lookups may name appended materials from the next
 * ycge_scene_attach_grids on. */
int ycge_scene_append_materials(ycge_ctx *ctx, const ycge_material *materials, int32_t n, int32_t *out_first_index);
/* The OBJ held by ycge_obj_parse, placed as ycge_obj_triangles (auto_ground = 0: normalize, target_size, scale, translate) or
 * ycge_obj_triangles_auto_ground (auto_ground = 1: scale, target; normalize and target_size are not read) places it, becomes a resident
 * mesh of material `material`: its triangle soup goes from the OBJ kernels' device buffer to the tree builder without crossing the bus
 * (read back once where the host builder has to build the tree).  The same index, bounds and pixels as that call followed by
 * ycge_scene_attach_meshes; out_bounds (or NULL) and out_mesh_index are written only on success. */
int ycge_scene_attach_obj_mesh(ycge_ctx *ctx, int32_t auto_ground, int32_t normalize, float target_size, float scale, const float translate_or_target[3],
                               int32_t material, int32_t *out_mesh_index, float out_bounds[6] /* or NULL */);

/* --- chunk generation: the chunks ycge_scene_attach_grids receives come from WorldGenerator.GenerateChunkCells on the host's worker threads
 * (WorldManager.cs:754-793, 914; 2 312 calls before the first frame when there is no world file, VolumeScenes.cs:617-624).  The function is
 * pure - (cx, cy, cz, WorldConfig) in, the (int,int)[S,S,S] of ycge_grid.cells out - so a chunk can be made where it will be traced.
 * Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing struct changes; a host detects these exports by symbol lookup.
 * The generator is the per-chunk one (WorldGenerator.cs:95-203: TerrainNoise, RiverNetwork.ComputeForChunk, BiomeMap, Layering, StrataMap,
 * FloraPlacer.PlaceTreesInChunk) with IslandSettings and WorldGenSettings at the reference's values; the whole-world pregen path
 * (GenerateAndSaveWorld) is a different function: ycge_worldgen_world_cells / ycge_scene_generate_world below.  MathF.Pow is
 * csrc/ycge_math.h's m_pow (within 1 ulp of a faithful libm), as everywhere in this library. */
typedef struct ycge_world {      /* WorldConfig (WorldConfig.cs:19-34), the fields a chunk depends on */
    int32_t chunk_size;          /* ChunkSize, 4..64                                          */
    int32_t chunks_y;            /* ChunksY >= 1: WorldHeight = chunks_y * chunk_size; WaterLevel and SnowLevel follow as :32-33 */
    int32_t world_seed;          /* WorldSeed                                                 */
    ycge_vec3 world_min;         /* WorldMin: chunk (cx, cy, cz) has min_corner world_min + c * chunk_size * voxel_size (WorldManager.cs:761-768) */
    ycge_vec3 voxel_size;        /* VoxelSize                                                 */
} ycge_world;
/* GenerateChunkCells on the host, one thread: pure host code, no context and no device.  cells_out: 2 * chunk_size^3 int32 in
 * ycge_grid.cells order; *any_solid_out = 1 when a cell is not Air, else 0.  YCGE_ERR_INVALID_ARG: a NULL pointer, chunk_size outside
 * 4..64, chunks_y < 1 or a world higher than 2^20, a key outside +-2^24 blocks (|c| * chunk_size: block coordinates must be exact in
 * binary32) - the same checks ycge_scene_generate_grids makes. */
int ycge_worldgen_chunk_cells(const ycge_world *world, int32_t cx, int32_t cy, int32_t cz, int32_t *cells_out, int32_t *any_solid_out);
/* Generate n chunks ON THE DEVICE (csrc/ycge_worldgen.hip) and make them resident: what ycge_scene_attach_grids gives when it is handed,
 * for the same keys in the same order, the cells ycge_worldgen_chunk_cells returns - the same pixels, indices, limits and statuses, all or
 * nothing, joining the frames in flight, forwarded to the devices of a one-process multi-device context, as documented there.
 *   keys = n x {cx, cy, cz}; a key may appear more than once (each takes a grid).
 *   proto: a ycge_grid whose `cells` is ignored; its lookup table, default_material and wireframe settings serve every chunk; nx, ny, nz
 *     and min_corner are overwritten per chunk (chunk_size; WorldManager.cs:761-769), voxel_size is the world's.
 *   A chunk with no cell other than Air takes no slot and reports index -1 (WorldManager.cs:759).
 *   The keys are worked through in internal sub-batches bounded by the staging area; a failure in any of them leaves the scene as it was
 *     and out_grid_index untouched.
 *   cells_out, when not NULL, receives the raw cells of every chunk (n * 2 * chunk_size^3 int32) - the only bulk read-back; a host leaves
 *     it NULL.  It may have been written when the call is refused later.
 *   YCGE_WORLDGEN_HOST in the environment at ycge_create: the cells are made by the host generator and go up as an attach's. */
int ycge_scene_generate_grids(ycge_ctx *ctx, const ycge_world *world, const int32_t *keys /* 3 n */, int32_t n, const ycge_grid *proto,
                              int32_t *out_grid_index /* n */, int32_t *cells_out /* NULL, or n * 2 * chunk_size^3 */);

/* --- the pregenerated world: VolumeScenes.BuildMinecraftLike with a file name never calls the per-chunk generator; it builds the whole
 * world with WorldManager.GenerateAndSaveWorld (WorldManager.cs:510-631), reads the file back and attaches every chunk
 * (VolumeScenes.cs:608-616).  That function differs from GenerateChunkCells: rivers over the whole map (RiverNetworkGlobal: a cell with no
 * lower neighbour adds nothing), slope / D8 / flora clamped at the WORLD's edge, the bank rule (wY - gY) <= 3.5f, and
 * FloraPlacer.PlaceTreesGlobal (trees cross chunk borders, another trunk clip, no slope test, cacti and (Stone, 1) rock piles in deserts).
 * Found by symbol lookup as the two above; YCGE_ABI_VERSION stays 10.
 *   The WINDOW: chunks_x x chunks_y x chunks_z chunks of chunk_size; nx = chunks_x * S, ny = chunks_y * S, nz = chunks_z * S.  Column
 *     (x, z) of the window is block (origin_bx + x, origin_bz + z) in every noise, hash and strata call; every edge clamp and bound is the
 *     window's.  origin (0, 0) is the reference's world, bit for bit.
 *   YCGE_ERR_INVALID_ARG, nothing written: what ycge_worldgen_chunk_cells refuses of `world`, chunks_x or chunks_z < 1, a window whose block
 *     coordinates leave +-2^24, nx * ny * nz >= 2^30, a NULL cells_out.
 * ycge_worldgen_world_cells: GenerateAndSaveWorld's worldCells on the host, one thread, no context and no device.  cells_out: 2*nx*ny*nz
 * int32 in the VG01 payload order (x, then y, then z; {mat, meta}) - what bw.Write emits at :616-628. */
int ycge_worldgen_world_cells(const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t *cells_out);
/* The same world made ON THE DEVICE (csrc/ycge_worldpregen.hip) and made resident: what ycge_scene_attach_grids gives when handed, chunk by
 * chunk in (cx, cy, cz) order with cx outermost, the S^3 slices of ycge_worldgen_world_cells' result - the same pixels, indices, limits and
 * statuses, all or nothing, joining the frames in flight, forwarded to the devices of a one-process multi-device context.
 *   Chunk (cx, cy, cz) gets min_corner = world_min + c * S * voxel_size.  A chunk none of whose cells is other than Air - after the flora
 *     pass, whose trees cross chunk borders - takes no slot and reports -1 (AttachChunkFromPreloaded, WorldManager.cs:704-720).
 *   out_grid_index: chunks_x * chunks_y * chunks_z, in that order; untouched when the call is refused.
 *   proto: as for ycge_scene_generate_grids.  The chunks are worked through in sub-batches bounded by the staging area.
 *   cells_out: NULL, or the whole world as ycge_worldgen_world_cells writes it (the only bulk read-back).  Untouched by an argument
 *     refusal (the list above, a bad proto, no scene); it may have been written when the call is refused later.
 *   YCGE_WORLDGEN_HOST at ycge_create (or a lookup table k_grid_encode does not take): ycge_worldgen_world_cells makes the cells and they
 *     go up as an attach's. */
int ycge_scene_generate_world(ycge_ctx *ctx, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz,
                              const ycge_grid *proto, int32_t *out_grid_index /* chunks_x*chunks_y*chunks_z */, int32_t *cells_out /* NULL, or 2*nx*ny*nz */);

/* --- the world store: a host that HAS a VG01 world file reads it into preloadedWorld once (WorldManager.ReloadFromExistingFile,
 * WorldManager.cs:399-508), and from then on every chunk that enters the view is a slice of that array (AttachChunkFromPreloaded, :696-752,
 * from EnsureViewLoaded, EnsureAllChunksLoaded and the LoadChunksAround tick).  Here the payload goes up ONCE and stays resident on the
 * device; chunks are attached from it by key and no cell crosses the bus again (csrc/ycge_world_store.cpp, kernels in
 * csrc/ycge_world_store.hip).  Found by symbol lookup as the exports above; YCGE_ABI_VERSION stays 10.
 *   The store belongs to the context, not to the scene: ycge_scene_upload keeps it, ycge_world_store_release and ycge_destroy free it, a
 *     second ycge_world_store_load replaces it - once the new one is complete: a refused or failed load leaves the old store as it was.  Grids
 *     attached from a store are encoded copies and stay resident when it goes.  A load touches no scene and joins no frame in flight.
 *   One-process multi-device: every device holds the payload; a peer context is refused by all of these.
 *   YCGE_WORLD_STORE_SLAB_BYTES at ycge_create (default 64 MiB): the payload goes up in slabs of whole x-planes (one at least) through two
 *     page-locked staging buffers of that size, the copy of one slab beside the occupancy kernel on the one before; a `cells` range that is
 *     page-locked already (ycge_alloc_host_buffer, ycge_pin_host_buffer) is copied from directly.
 *   YCGE_WORLD_STORE_HOST at ycge_create: the store is a host copy, chunks are sliced by a host loop and go up as an attach's cells do. */
/* The header of a VG01 file as ReloadFromExistingFile checks it (:414-424): 'V','G','0','1', little-endian int32 nx, ny, nz, the payload at
 * offset 16.  Pure host code, no context and no device.  YCGE_ERR_INVALID_ARG with the reference's text in msg (may be NULL):
 * "Unsupported world file header. Expected 'VG01'.", "Invalid world dimensions.", "Unable to read beyond the end of the stream." (n_bytes
 * below 16 or below 16 + 8 * nx * ny * nz); also refused: nx * ny * nz >= 2^30 (ycge_scene_generate_world's limit), a NULL bytes or dims_out. */
int ycge_world_file_info(const uint8_t *bytes, size_t n_bytes, int32_t dims_out[3], size_t *payload_offset_out /* may be NULL */, char *msg, size_t msg_bytes);
/* Make the payload resident.  cells: 2 * nx * ny * nz int32, x, then y, then z fastest, {mat, meta} - it may point into a mapped file and is
 * not read after the call.  Per chunk of chunk_size, clipped at the far faces (:698-700), the load finds whether any cell has mat != 0 (:716).
 * YCGE_ERR_INVALID_ARG: a NULL pointer, a dimension < 1, nx * ny * nz >= 2^30, chunk_size outside 1..1024, more than 2^24 chunks, a peer
 * context.  An allocation failure is YCGE_ERR_OUT_OF_MEMORY, as for ycge_scene_attach_grids. */
int ycge_world_store_load(ycge_ctx *ctx, const int32_t *cells, int32_t nx, int32_t ny, int32_t nz, int32_t chunk_size);
/* The store's dimensions, chunk size (either may be NULL) and, when occupied_out is not NULL, one byte per chunk in (cx, cy, cz) order with
 * cx outermost (ceil(n / chunk_size) chunks per axis): 1 when a cell of the chunk has mat != 0.  YCGE_ERR_INVALID_ARG with a message:
 * no store, or capacity below the number of chunks. */
int ycge_world_store_info(ycge_ctx *ctx, int32_t dims_out[3], int32_t *chunk_size_out, uint8_t *occupied_out, size_t capacity);
/* Attach n chunks of the store by key: what ycge_scene_attach_grids gives when it is handed, for the same keys in the same order, the cells
 * AttachChunkFromPreloaded slices - the same pixels, indices, limits and statuses, all or nothing, joining the frames in flight, forwarded
 * to the devices of a one-process multi-device context, as documented there.
 *   proto: as for ycge_scene_generate_grids, but proto->min_corner is WorldMin and proto->voxel_size is VoxelSize: chunk (cx, cy, cz) gets
 *     nx, ny, nz = its clipped sizes and min_corner = WorldMin + (float)(c * chunk_size) * VoxelSize in binary32 (:720-724).
 *   No slot, index -1: a key with a negative component or at or beyond the chunk counts (the reference indexes out of range there, and
 *     EnsureViewLoaded swallows it), and a chunk with no cell of mat != 0.  A chunk whose only non-zero ids are negative DOES take a slot:
 *     the reference attaches it (!= 0) although VolumeGrid draws nothing of it (matId > 0).  A key may repeat; each occurrence takes a grid.
 *   YCGE_ERR_NO_SCENE before the first upload; YCGE_ERR_INVALID_ARG with a message when there is no store.  A pair with no material and
 *     default_material < 0 is refused as the attach refuses it; the message names the chunk key and the cell in the chunk. */
int ycge_scene_attach_world_chunks(ycge_ctx *ctx, const int32_t *keys /* 3 n */, int32_t n, const ycge_grid *proto, int32_t *out_grid_index /* n */);
/* Free the store on every device (YCGE_OK when there is none). */
int ycge_world_store_release(ycge_ctx *ctx);
/* Make the window of ycge_scene_generate_world the context's world store, ON THE DEVICE: the reference's start-up path is
 * GenerateAndSaveWorld, ReloadFromExistingFile, LoadChunksAround - here generate, (ycge_world_store_read to save,) and attach by key, with
 * no cell of the world on the bus.  world, chunks_x, chunks_z, origin_bx, origin_bz: as for ycge_scene_generate_world, with its limits and
 * refusals; the store's dimensions are chunks * chunk_size per axis and its chunk size is world->chunk_size.  The store's rules above hold:
 * it belongs to the context, the call touches no scene and joins no frame in flight, it replaces an older store (loaded or generated) only
 * once it is complete, a refused or failed call leaves the old store as it was, a peer context is refused, every device of a one-process
 * multi-device context makes its own copy.  Found by symbol lookup; YCGE_ABI_VERSION stays 10.
 *   form = YCGE_WORLD_STORE_FIELDS: what stays resident is the 2-D fields of the window - column records, feature descriptors, the settled
 *     anyLeaves fallback flags, the features' reach: tens of bytes a column, where a cell store takes 8 bytes a cell - and the chunk
 *     occupancy.  No 3-D array of the world exists anywhere; ycge_scene_attach_world_chunks makes each chunk's cells from the fields when its
 *     key is attached (k_wp_fill), under the same contract word for word, and ycge_world_store_read makes planes (k_wp_planes).
 *   form = YCGE_WORLD_STORE_CELLS: the ordinary device cell store, its payload written on the device by k_wp_planes in slabs of
 *     YCGE_WORLD_STORE_SLAB_BYTES; afterwards indistinguishable from ycge_world_store_load of ycge_worldgen_world_cells' result.
 *   Any other form: YCGE_ERR_INVALID_ARG.
 *   YCGE_WORLDGEN_HOST or YCGE_WORLD_STORE_HOST at ycge_create: ycge_worldgen_world_cells makes the cells on the host and the store is what
 *     ycge_world_store_load makes of them (with YCGE_WORLD_STORE_HOST: a host copy), whatever the form. */
#define YCGE_WORLD_STORE_FIELDS 0
#define YCGE_WORLD_STORE_CELLS 1
int ycge_world_store_generate(ycge_ctx *ctx, const ycge_world *world, int32_t chunks_x, int32_t chunks_z, int32_t origin_bx, int32_t origin_bz, int32_t form);
/* The x-planes [x0, x0 + planes) of the store in VG01 payload order - x, then y, then z fastest, {mat, meta}: what bw.Write emits at
 * WorldManager.cs:616-628 - so a host writes the 16 header bytes and then the payload slab by slab.  Any store: a host copy is copied, a
 * device cell store is copied through page-locked staging (directly into a page-locked cells_out), a fields store makes the planes in a
 * device slab first.  It may wait for the frames in flight and changes no later frame.  YCGE_ERR_INVALID_ARG with a message: no store,
 * planes < 1, a range outside 0..nx, a NULL cells_out, a peer context; nothing is written then.  Found by symbol lookup. */
int ycge_world_store_read(ycge_ctx *ctx, int32_t x0, int32_t planes, int32_t *cells_out /* 2 * planes * ny * nz */);

/* --- voxel edits: a host that digs or places a block changes cells of a grid that is resident, and of the world store, where they lie.
 * Without these two calls the route is a host copy of every chunk's raw cells, a detach, an attach of the whole chunk and an objects
 * update - and the store has no route at all.  The reference has no block editing: the existing paths define the result.  Added after
 * ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing struct changes; a host detects both exports by symbol lookup.
 * An op sets every cell of an inclusive index box to one (mat_id, meta_id) pair.  Ops apply in list order: where boxes overlap, the
 * later op wins. */
typedef struct ycge_voxel_edit {   /* 9 int32, 36 bytes */
    int32_t grid_index;            /* resident grid; must be 0 for ycge_world_store_edit */
    int32_t lo[3], hi[3];          /* inclusive index box; one cell is lo == hi          */
    int32_t mat_id, meta_id;       /* the pair every cell of the box becomes             */
} ycge_voxel_edit;
#define YCGE_VOXEL_EDIT_MAX_OPS (1 << 20)
/* Edit cells of resident grids (those of the upload and attached ones alike), on the device, in place.
 *   Same pixels.  After the call every frame, every ycge_read_buffer buffer, every scene query, the counting instances' counters and
 *     ycge_read_timed_steps are what the same context gives after one ycge_scene_upload of the equivalent scene instead - the same
 *     materials, the same Scene.Objects in the same order, the grids with the ops applied to their cells - bit for bit, TAA history and
 *     exposure state included.  Cell codes and offsets are internal and may differ.
 *   Complete scene.  The call leaves a complete, renderable scene on its own; no ycge_scene_update_objects has to follow.  An object
 *     record carries its grid's solid box and the walk tree is derived from it, so whenever an edit changes the record of a grid that an
 *     object holds (its solid box or its brick mask), the call installs the objects again as ycge_scene_update_objects does, from the
 *     context's own copy of the last object list ycge_scene_upload or ycge_scene_update_objects accepted.  An edit that leaves every
 *     record as it was - the common dig or place inside the box - only touches bytes.
 *   out_info (4 words, or NULL): cells whose code differs from before the call, bricks that hold such a cell, grids whose record
 *     changed, objects installed again (0 or 1).  Written only on success.
 *   Codes.  A cell is one byte, a code into the grid's material table.  mat_id <= 0 is air with any meta_id.  A grid that the device
 *     encoded (an attached grid whose lookup table has at most 254 entries) is coded by its lookup table: 1 + the first matching entry,
 *     or the code of default_material for a pair the table lacks - such a grid has NO limit of distinct pairs under edits.  A grid that
 *     the host encoded (the grids of an upload; an attached grid with a larger lookup table) numbers its pairs as they first appear: a
 *     new pair takes the next free code and its table entry is written; a 256th code is refused with YCGE_ERR_UNSUPPORTED.  Codes of
 *     pairs no cell holds any more are not reclaimed (the message says so): detaching the grid and attaching it again is the way out.
 *   Refusals are decided on the host before any device work and are all or nothing: nothing is written, scene and pool stay as they
 *     were.  YCGE_ERR_INVALID_ARG with a message that names the op: NULL ops with n > 0, n < 0, n > YCGE_VOXEL_EDIT_MAX_OPS, a grid that is
 *     not resident, lo > hi on an axis, a box that leaves the grid, a solid pair with no material (the lookup table lacks it and
 *     default_material < 0; the message names the pair too).  YCGE_ERR_INVALID_ARG for a peer context, YCGE_ERR_NO_SCENE before the
 *     first upload.  n = 0 is YCGE_OK.
 *   Frames in flight are joined (they read the cells).  Scene queries see the edit with the next query.
 *   One-process multi-device: the root forwards to every device, as an attach does; a peer context refuses.  Tiled ranks each make the
 *     same call.
 * The host turns every op into a code byte and lists the bricks the boxes touch; one workgroup per brick rewrites the bytes, a second
 * kernel reduces the edited grids' solid boxes and brick masks, one small read-back follows (csrc/ycge_grid_edit.hip). */
int ycge_scene_edit_voxels(ycge_ctx *ctx, const ycge_voxel_edit *ops, int32_t n, uint32_t *out_info /* 4 words or NULL */);
/* Edit cells of the world store.  Boxes are in store cell coordinates - x, y, z of the VG01 payload - and grid_index must be 0.  The
 * raw pairs are written as given, with any values.  The occupancy of every chunk an op touches is found again (mat != 0), the clipped
 * chunks of the far faces included: a chunk may become empty - an attach of its key then reports -1 - or occupied.  Afterwards the
 * store is what ycge_world_store_load of the edited cells gives, to ycge_world_store_read, ycge_world_store_info and
 * ycge_scene_attach_world_chunks alike.  A device cell store is edited by kernels, a YCGE_WORLD_STORE_HOST store by a host loop; a
 * YCGE_WORLD_STORE_FIELDS store holds no cells and refuses with YCGE_ERR_UNSUPPORTED (generate with YCGE_WORLD_STORE_CELLS instead) -
 * unless it has a pool of materialised chunks (ycge_world_store_reserve_edits, below), which changes nothing else of this contract.
 * No scene is touched: grids attached earlier are encoded copies and keep their cells (edit those with ycge_scene_edit_voxels).  The
 * call waits for frames in flight only where ycge_world_store_read would.  Every device of a multi-device context edits its own copy.
 * Refusals as above, all or nothing, the message names the op; in addition: no store, grid_index != 0, a box that leaves the store. */
int ycge_world_store_edit(ycge_ctx *ctx, const ycge_voxel_edit *ops, int32_t n);
/* --- edits on a YCGE_WORLD_STORE_FIELDS store: a pool of materialised chunks beside the fields, copy-on-write at chunk granularity.  A
 * played world edits a few hundred chunks of thousands, so the fields stay and cells exist only for chunks that were edited.  Found by
 * symbol lookup; YCGE_ABI_VERSION stays 10, no existing struct changes.
 * ycge_world_store_reserve_edits gives the context's fields store a pool of max_chunks slots of S^3 cells (S: the chunk size), 8 bytes a
 * cell in ycge_grid.cells order: max_chunks * S^3 * 8 bytes ON EVERY DEVICE of a one-process multi-device context (each holds its own
 * pool; a peer context is refused).  A generated store's dimensions are whole chunks, so no slot is clipped.  A later call with another
 * count resizes the pool and keeps the slots in use.  ycge_world_store_release and a new ycge_world_store_load or _generate drop the
 * pool with the store.
 *   Refusals are all or nothing - the store and an earlier pool stay as they were.  YCGE_ERR_INVALID_ARG with a message: no store, a
 *     store that is not in the fields form (it holds its cells and needs no pool; YCGE_WORLDGEN_HOST and YCGE_WORLD_STORE_HOST make such
 *     a store whatever the form asked for), max_chunks < 1, above the store's chunk count or below the slots in use.
 *     YCGE_ERR_OUT_OF_MEMORY: an allocation that fails.
 * With a pool ycge_world_store_edit makes every check it makes on a cell store, in the same order, on the host before any device work.
 *   Then EVERY CHUNK AN OP TOUCHES TAKES A SLOT and keeps it - also when the pair written equals what the generator made; nothing
 *   reclaims a slot but ycge_world_store_revert_chunks.  There are two ways to run out of slots: the pool is smaller than the number of
 *   distinct chunks the host edits over time (grow it with a larger max_chunks, or revert chunks), or one call's ops touch more chunks
 *   without a slot than slots are free.  Such a call is refused as a whole with YCGE_ERR_OUT_OF_MEMORY and nothing is written; the message
 *   names the first op that does not fit and gives both counts.  Otherwise the new slots' chunks are made from the fields (k_wp_fill, a
 *   launch per batch of chunks), the ops - clipped against the chunks they touch - are applied in list order with the later winning
 *   (k_ws_pool_edit), the touched slots' occupancy is found again (k_ws_pool_occupied) and one small read-back follows.  YCGE_WS_POOL_BATCH
 *   at ycge_create (default and most 32768) bounds the records of one such launch.
 * Every reader sees the pool: to ycge_world_store_read (k_ws_pool_planes over k_wp_planes' slab), ycge_world_store_info and
 *   ycge_scene_attach_world_chunks (a chunk that holds a slot is copied out of it, in one batch with chunks made from the fields; an
 *   emptied chunk reports -1, a generated-empty chunk that an edit made solid attaches) the store is what a YCGE_WORLD_STORE_CELLS store
 *   of the same world and window is after the same ycge_world_store_edit calls. */
int ycge_world_store_reserve_edits(ycge_ctx *ctx, int32_t max_chunks);
/* The pool's slots and how many of them hold a chunk (either may be NULL); 0 and 0 for a store without a pool and for no store. */
int ycge_world_store_edit_slots(ycge_ctx *ctx, int32_t *capacity_out, int32_t *used_out);
/* Give the slots of these chunks back: each is the generated chunk again, its cells and its occupancy, to every reader.  A key that
 * holds no slot (or repeats) is not an error, nor is a store without a pool.  No device work.  YCGE_ERR_INVALID_ARG, nothing changed: no
 * store, a NULL keys with n > 0, n < 0, a key outside the chunk counts (the message names the key), a peer context. */
int ycge_world_store_revert_chunks(ycge_ctx *ctx, const int32_t *keys /* 3 n */, int32_t n);

/* The argument checks of ycge_scene_upload on their own: pure host code, no device and no context needed
 * (every index in range, counts non-negative, pointers present, material kinds known).  Returns YCGE_OK or the
 * status ycge_scene_upload would return; `msg` (may be NULL) receives the reason. */
int ycge_validate_scene(const ycge_scene *scene, char *msg, size_t msg_bytes);

/* Resize(fb, ss)   RaytraceEntity.cs:289; drops TAA history (RaytraceRenderer.cs:137) */
int ycge_resize(ycge_ctx *ctx, int32_t fb_width, int32_t fb_height, int32_t super_sample);
/* SetCamera(pos,yaw,pitch) + SetFov(deg)   RaytraceEntity.cs:229,99 */
int ycge_set_camera(ycge_ctx *ctx, const float pos[3], float yaw, float pitch, float fov_deg);

/* TryFlipAndBlit(fb)   RaytraceEntity.cs:230 / RaytraceRenderer.cs:157-267.
 * out_top_bottom_sdr: fbW*fbH*2*3 f32, caller-owned host memory, per chexel
 * {top rgb, bottom rgb}; the host then does fb.SetChexel(cx,cy,new Chexel('▀',
 * top, bottom)) unchanged (RaytraceRenderer.cs:260-261).  May be NULL (frame is
 * still rendered; read buffers with ycge_read_buffer).  stats may be NULL. */
int ycge_render_frame(ycge_ctx *ctx, float *out_top_bottom_sdr, ycge_frame_stats *stats);
/* Frames in flight (no counterpart in the reference, whose TryFlipAndBlit returns a finished frame): queues steps 1-5 and 9 of the
 * next frame - camera snapshot, trace, TAA, camera commit - and returns without waiting.  The trace of frame N + 1 runs beside the
 * TAA of frame N (its own stream; three sets of trace outputs taken in turn) and two traces run at a time on two streams - the
 * single-launch kernel always, the stage pipeline of voxel worlds from 4096 tiles on and with no post stage in flight (a second set
 * of stage queues) - so a sequence of such calls costs max(trace, TAA + schedule) per frame or less, instead of their sum plus the
 * host's wake-up.  The frames are the ones the same sequence of ycge_render_frame(ctx, NULL, NULL)
 * calls produces, bit for bit.  Single device, no debug captures, no per-frame counters.  Every other entry point (and
 * ycge_wait) first waits for the frames in flight - except the scene queries ycge_scene_hit / ycge_scene_occluded, which run beside
 * them; ycge_set_camera between two calls moves the camera of the next frame. */
int ycge_render_frame_async(ycge_ctx *ctx);
/* ... with steps 6-8 (denoise, exposure, tonemap + downsample) and the read-back: out_top_bottom_sdr (as for ycge_render_frame) is
 * filled when the frame is complete - after ycge_wait or any other call - so a caller that queues several such frames passes one
 * buffer per frame in flight (page-locked, ycge_pin_host_buffer, or the copy blocks the calling thread).  The post stage of frame N
 * runs beside the traces and TAA of the frames after it; same pixels as ycge_render_frame(ctx, out, NULL) in the same order. */
int ycge_render_frame_async_sdr(ycge_ctx *ctx, float *out_top_bottom_sdr);
/* --- device chexel colours: the presenters' colour maps computed beside the tonemap, so that a host reads back the bytes it presents
 * instead of 24 bytes of f32 a chexel and maps them itself.  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10 and
 * ycge_config is unchanged - a host detects these two exports by symbol lookup.  Per chexel (index cx + cy * fbW), from the SDR
 * {top rgb, bottom rgb} that ycge_render_frame writes, exactly as the reference maps it:
 *   out_color16  fbW * fbH bytes: color_16 of top | color_16 of bottom << 4 - ChexelColor(Vec3) (Renderer/Chexel.cs:37-41, 70-99),
 *                the low byte of Win32's MapAttributes(fg = top, bg = bottom)
 *   out_ansi     fbW * fbH * 2 bytes {top, bottom}: ChexelToAnsi256 (Renderer/ANSITerminalRenderer.cs:246-306)
 *   out_rgba     fbW * 2 fbH RGBA8 (alpha 255), row 2 cy the top half-cell, row 2 cy + 1 the bottom one: OpenGLTerminalRenderer's
 *                compose image (:114-145, LinearToSrgb8 :390-400) for a framebuffer that fills the window
 * Any subset of the four destinations (out_top_bottom_sdr as for ycge_render_frame) may be NULL, not all of them.
 * The synchronous call is ycge_render_frame with the post stage run whatever the destinations: the same SDR, bit for bit, and the same
 * frame state (counter, TAA history, exposure) as ycge_render_frame(ctx, sdr, stats) in its place; the one-process multi-device forms
 * included.  Refused: all destinations NULL, a peer context, the RCCL exchange with lean slabs (config.slab_albedo = 0).
 * The frames-in-flight call mirrors ycge_render_frame_async_sdr; every destination must be page-locked memory.  No destination of
 * a refused or failed call is written later. */
int ycge_render_frame_chexels(ycge_ctx *ctx, float *out_top_bottom_sdr, uint8_t *out_color16, uint8_t *out_ansi, uint8_t *out_rgba,
                              ycge_frame_stats *stats);
int ycge_render_frame_async_chexels(ycge_ctx *ctx, float *out_top_bottom_sdr, uint8_t *out_color16, uint8_t *out_ansi, uint8_t *out_rgba);
/* --- the ANSI presenter's escape stream on the device: the bytes ANSITerminalRenderer.Render() (Renderer/ANSITerminalRenderer.cs:86-153)
 * writes for a console_w x console_h console whose only framebuffer is this context's fbW x fbH at (viewport_x, viewport_y) - built from
 * the ANSI pairs of ycge_render_frame_chexels, which stay on the device, by one prefix sum over the cells.  Added after ABI 10 without
 * changing it: a host detects these exports by symbol lookup.
 *   [ESC[2J ESC[H when clear_screen], per row ESC[<y+1>;1H, per cell the SGR escape of the indices that differ from the previous cell's
 *   (ESC[38;5;F;48;5;Bm / ESC[38;5;Fm / ESC[48;5;Bm / none; (-1, -1) before the first cell, rows included) and its character, ESC[0m.
 *   A covered cell is ('\u2580', ansi(top), ansi(bottom)); any other is (' ', ansi(palette[default_fg16]), ansi(palette[default_bg16])).
 * ycge_ansi_stream_bound: 7 + 4 + sum over rows of (5 + digits(y + 1)) + 23 console_w console_h bytes - no context, no device.
 * ycge_render_frame_ansi: the frame state and the optional SDR are ycge_render_frame's, bit for bit; *out_len bytes of out_stream are
 * written, never a byte past them.  Refused before any device work, the frame state unchanged: NULL out_stream or out_len, a console
 * that is not positive or whose bound reaches 2^32, defaults outside 0..15, capacity below the bound, a peer context, the RCCL exchange
 * with lean slabs.  A failed or refused call writes nothing to the caller's arrays, then or later. */
int ycge_ansi_stream_bound(int32_t console_w, int32_t console_h, size_t *bytes);
int ycge_render_frame_ansi(ycge_ctx *ctx, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                           int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len,
                           float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
/* --- Video mode: the other renderer behind the reference's IConsoleRenderer seam (RaytraceEntity.cs:12-50, VideoWrapper -> VideoRenderer),
 * for a host that presents through the device encoders and must not fall back to CPU threads when the user switches to a camera or a
 * video.  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no struct changes; a host detects these exports by symbol lookup.
 * ycge_video_blit is VideoRenderer.TryFlipAndBlit (Renderer/VideoRenderer.cs:68-148) for the frame IFrameReader.GetCurrentFramePtr() shows:
 * src_w x src_h pixels of bytes_per_pixel = 3 (BGR) or 4 (BGRA, the 4th byte ignored), row-major, no row padding - letterboxed into the
 * context's hi-res grid (fbW, fbH, ss of ycge_create / ycge_resize: hiW = fbW*ss, hiH = fbH*2*ss), each hi-res sample a 6 x 6 Lanczos-3
 * resample, ss*ss samples averaged per half-cell.
 *   Same pixels: out_top_bottom_sdr is, bit for bit, the {topAvg, botAvg} that VideoRenderer.cs:127-128 passes to new Chexel('\u2580', ...), in
 *   the layout of ycge_render_frame.  out_color16 / out_ansi / out_rgba are what ycge_render_frame_chexels gives for those values, and the
 *   stream of ycge_video_blit_ansi is what ycge_render_frame_ansi gives for those pairs (arguments, bound, refusals and output as there).
 *   The weights come from the C library's sinf (MathF.Sin).  The reference's bilinear fallback (:215: a weight sum <= 0) is not implemented:
 *   no geometry is known to reach it, and one that did fails with YCGE_ERR_INTERNAL instead of showing other pixels.
 *   No scene needed: a context that never saw ycge_scene_upload blits.
 *   Frame state untouched: a blit changes nothing a ray-traced frame reads - frame counter, TAA history, exposure state, trace outputs,
 *   schedule, statistics.  It first waits for the frames in flight, like every entry point except the scene queries, and returns with the
 *   destinations filled; `frame` is the caller's own again then.  There is no frames-in-flight form of the blit (deliberately: a video
 *   frame is a copy and one short launch, there is nothing to overlap it with).
 *   Geometry follows ycge_resize (VideoWrapper.Resize makes a new VideoRenderer).
 *   A pageable `frame` goes up through page-locked staging of the library; a page-locked one (ycge_alloc_host_buffer, ycge_pin_host_buffer)
 *   goes up directly.  Destinations as for ycge_render_frame_chexels: any subset may be NULL, not all of them.
 *   Refused before any device work with YCGE_ERR_INVALID_ARG, nothing written then or later, the context usable: NULL frame, src_w or
 *   src_h < 1, bytes_per_pixel not 3 or 4, src_w*src_h*bytes_per_pixel >= 2^31, all destinations NULL, a peer context of the one-process
 *   multi-device form (its root blits on devices[0]); for the stream form also NULL out_stream or out_len, a console that is not positive
 *   or whose bound reaches 2^32, defaults outside 0..15, capacity below ycge_ansi_stream_bound. */
int ycge_video_blit(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                    float *out_top_bottom_sdr, uint8_t *out_color16, uint8_t *out_ansi, uint8_t *out_rgba);
int ycge_video_blit_ansi(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                         int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                         int32_t default_fg16, int32_t default_bg16, int32_t clear_screen,
                         uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr /* may be NULL */);
/* --- The delta ANSI stream: only the cells that changed since the last stream this context handed out.  The reference has no delta
 * presenter, so these rules define the bytes; they are tied to Render() in two ways: a keyframe IS the stream of ycge_render_frame_ansi, and
 * a delta applied to a terminal that shows the previous stream leaves it showing what the full stream of the new frame would, with the
 * cursor and the SGR state where the full stream leaves them (Terminal.Start writes its HUD right behind Render()).  Added after ABI 10
 * without changing it: a host detects these exports by symbol lookup.
 *   Geometry, covered cells and default cells are those of ycge_render_frame_ansi.  `prev` is the pair array of the last stream this
 *   context handed out successfully through either export below, `cur` this frame's.
 *   Keyframe: the stream of ycge_render_frame_ansi (ycge_video_blit_ansi) for the same arguments, byte for byte.  Returned when there is no
 *   valid prev, when the geometry key {console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, fbW, fbH} differs from
 *   that of prev, when clear_screen != 0 or when keyframe != 0.
 *   Delta, with merge_gap = G in 0..8:
 *     changed(x, y): the cell is covered and its pair differs from prev in either byte.
 *     emitted(x, y): changed(x, y); or the cell lies in the same row strictly between two changed cells a < x < b with b - a - 1 <= G; or
 *       it is the console's last cell (console_w - 1, console_h - 1), covered or not - so the cursor ends exactly where the full stream
 *       leaves it, pending wrap included.
 *     Emitted cells are written in raster order.  An emitted cell is a run start when x == 0 or (x - 1, y) is not emitted: it writes
 *     ESC[<y+1>;<x+1>H, then ESC[38;5;<fg>;48;5;<bg>m unconditionally (Render()'s first branch against (-1, -1)).  Any other emitted cell
 *     writes the escape of Render()'s three branches (ANSITerminalRenderer.cs:120-143) against the pair of (x - 1, y).  Then the cell's
 *     character: '\u2580' in UTF-8 when covered, ' ' otherwise.  The stream ends with ESC[0m.  No clear prefix, no per-row ;1H moves.
 *   A delta never exceeds ycge_ansi_stream_bound, which stays the capacity to pass (the proof: csrc/ycge_ansi_cells.hip.h).
 *   out_info (4 words, or NULL): {keyframe returned (0 / 1), changed cells, emitted cells, run starts}; the three counts are 0 on a keyframe.
 *   State: prev advances only when one of these two calls returns YCGE_OK (two pair buffers are swapped, nothing is copied).  The next call
 *   is a keyframe after: a failure behind the call's refusals, ycge_resize, a change of the framebuffer size, a call to
 *   ycge_render_frame_ansi or ycge_video_blit_ansi on the context (the host has then shown something else).  A refusal of the call's
 *   arguments leaves the state as it was.  Both exports share the one delta state of the context: one terminal, whichever renderer the
 *   host shows on it (the mode switch of RaytraceEntity).
 *   The frame state, the SDR, the statistics and the refusals are those of ycge_render_frame_ansi / ycge_video_blit_ansi, and one more:
 *   merge_gap outside 0..8 is YCGE_ERR_INVALID_ARG, the message names the value.
 *   The host: write every stream it is handed to the terminal, in order and whole; pass keyframe = 1 (or clear_screen) after anything
 *   else wrote to the terminal's cells - a HUD line over the console area, another program, a redraw after a suspend. */
int ycge_render_frame_ansi_delta(ycge_ctx *ctx, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                 int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t keyframe, uint8_t *out_stream,
                                 size_t capacity, size_t *out_len, uint32_t *out_info /* 4 words or NULL */,
                                 float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_video_blit_ansi_delta(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                               int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                               int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t keyframe,
                               uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info /* 4 words or NULL */,
                               float *out_top_bottom_sdr /* may be NULL */);
/* --- 24-bit colour ANSI streams: the full, delta and video forms above on sRGB8 triples instead of palette indices, for terminals that take
 * ESC[38;2;R;G;Bm / ESC[48;2;R;G;Bm.  The reference has no 24-bit presenter, so these rules define the bytes; they are Render()'s
 * (ANSITerminalRenderer.cs:86-153) - the same walk, the same three branches, the same trailer - with "index" replaced by "sRGB8 triple".
 * Added after ABI 10 without changing it: a host detects these exports by symbol lookup.
 *   Colours.  A covered cell is ('▀', fg = RGB8(top), bg = RGB8(bottom)), RGB8 the three bytes ycge_render_frame_chexels writes for that
 *   half-cell into out_rgba (row 2 cy the top, row 2 cy + 1 the bottom).  Any other cell is (' ', RGB8(palette[default_fg16]),
 *   RGB8(palette[default_bg16])), from the same encoder run on the 16 palette colours.  Two colours are equal when all three bytes are.
 *   Full stream.  [ESC[2J ESC[H when clear_screen], per row ESC[<y+1>;1H, per cell against the previous cell in raster order (nothing before
 *   the first cell, rows included):
 *       both differ   ESC[38;2;R;G;B;48;2;R;G;Bm      fg only   ESC[38;2;R;G;Bm      bg only   ESC[48;2;R;G;Bm      neither   nothing
 *   then the character, and ESC[0m at the end.  Numbers as AppendInt writes them.
 *   Bound.  The longest escape is 7 + 11 + 6 + 11 + 1 = 36 bytes, a cell at most 36 + 3 = 39:
 *   ycge_ansi_rgb_stream_bound = 7 + 4 + sum over rows of (5 + digits(y + 1)) + 39 console_w console_h - no context, no device, refused as
 *   ycge_ansi_stream_bound refuses.  A console whose bound reaches 2^32 is refused by every stream call (offsets are 32-bit).
 *   Delta, with merge_gap = G in 0..8, keyframe as in ycge_render_frame_ansi_delta, and tolerance = T in 0..255:
 *     shown(x, y): the fg / bg pair of triples the terminal displays for a covered cell, according to the streams this context handed out
 *       through the two _rgb_delta exports.
 *     changed(x, y): the cell is covered and the largest |cur - shown| over its six channels exceeds T (T = 0: "differs").
 *     emitted, run starts and cursor moves are ycge_render_frame_ansi_delta's: gap merge inside a row only, the console's last cell always
 *       emitted, a run start writes ESC[<y+1>;<x+1>H and then the both-differ escape unconditionally; no clear prefix, no per-row moves;
 *       the trailer ESC[0m.  Any other emitted cell writes the three-branch escape against cur(x - 1, y): its left neighbour is emitted, so
 *       that is what the terminal holds there.
 *     After a successful call shown = cur for every emitted covered cell and is unchanged for every other; after a keyframe shown = cur.
 *     Guarantee: a terminal that shows the previous streams, fed this delta, ends with the cursor (pending wrap included) and the SGR state
 *       where the full stream of this frame leaves them, every cell's character the full stream's and every channel within T of the full
 *       stream's - identical when T = 0.  The error never accumulates: the comparison is against shown, not against the previous frame.
 *     (Why a tolerance: the 240-colour palette hid the +-1 flicker that TAA's running blend leaves in a resting picture; at 24 bits it would
 *     mark nearly every cell changed on every frame.)
 *   Keyframe: the full 24-bit stream for the same arguments, byte for byte - when there is no valid shown, when the geometry key
 *   {console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, fbW, fbH} differs, when clear_screen or keyframe is set.
 *   out_info as in ycge_render_frame_ansi_delta.  A delta never exceeds ycge_ansi_rgb_stream_bound (the same proof, with 39 for 23; the
 *   2 x 1 console with both cells changed and every channel three-digit reaches the bound less 7).
 *   State.  One terminal per context: the 24-bit delta state and the 256-colour delta state invalidate each other.  The next delta call of
 *   EITHER family is a keyframe after: any full stream of either family and either renderer, a delta of the other family, ycge_resize, a
 *   change of the framebuffer size, a failure behind the argument checks.  An argument refusal leaves the state untouched.  The ray-traced
 *   and the video 24-bit deltas share one state.  tolerance outside 0..255 is YCGE_ERR_INVALID_ARG, the message names the value.
 *   Everything else - the frame state, the SDR, the statistics, the refusals (peer context, RCCL with lean slabs, NULLs, capacity below the
 *   bound, defaults outside 0..15), "nothing written by a refused or failed call" - is the corresponding _ansi / _ansi_delta call's.  The
 *   RGBA plane stays on the device. */
int ycge_ansi_rgb_stream_bound(int32_t console_w, int32_t console_h, size_t *bytes);
int ycge_render_frame_ansi_rgb(ycge_ctx *ctx, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                               int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len,
                               float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_render_frame_ansi_rgb_delta(ycge_ctx *ctx, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                     int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance, int32_t keyframe,
                                     uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info /* 4 words or NULL */,
                                     float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_video_blit_ansi_rgb(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                             int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                             int32_t default_fg16, int32_t default_bg16, int32_t clear_screen,
                             uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr /* may be NULL */);
int ycge_video_blit_ansi_rgb_delta(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                                   int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                                   int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance,
                                   int32_t keyframe, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info /* 4 words or NULL */,
                                   float *out_top_bottom_sdr /* may be NULL */);
/* --- Quadrant glyphs in Video mode: the quadrant-glyph family (the rules: below, at ycge_render_frame_quadrants) for the frame a reader
 * shows, so that a host with quadrant glyphs on keeps the glyph family and the delta state across the switch to a camera or a film.  Added
 * after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing struct or prototype changes; a host detects the exports by symbol
 * lookup.  Each call is its video call's argument list with min_contrast where the frame form has it.
 *   Sub-cell colours.  super_sample = ss must be even.  The hi-res grid, the letterbox geometry, the two weight tables and every sample are
 *   ycge_video_blit's for the context's (fbW, fbH, ss); a sample is SampleSourceLanczos' value after its per-channel Clamp01
 *   (VideoRenderer.cs:184-241).  Quadrant k - 0 = TL, 1 = TR, 2 = BL, 3 = BR - of chexel (cx, cy) covers columns cx ss + (k & 1) ss / 2 ..
 *   + ss / 2 - 1 and rows (2 cy + (k >> 1)) ss .. + ss - 1.  Its colour: the binary32 sum of its samples, rows outer, columns inner, per
 *   channel, from 0, times 1.0f / (float)((ss / 2) ss), through Clamp01 - the blit's own average-and-saturate (:126-128) over half the columns.
 *   No tone map: a video frame has none.  out_quad_sdr in the frame call's layout, {TL rgb, TR rgb, BL rgb, BR rgb} a chexel.
 *   out_top_bottom_sdr is ycge_video_blit's array for the same frame, bit for bit: the serial sy, sx sum, not the quadrant sums' (in binary32
 *   the left and the right half do not add up to it).
 *   The fit, the glyph and the RGBA plane: the rules at ycge_render_frame_quadrants on these sub-cell colours, the bytes the chexel encoder's
 *   Clamp01 / LinearToSrgb8.  Destinations of ycge_video_blit_quadrants as there: any subset may be NULL, not all; pageable or page-locked.
 *   ycge_video_blit_ansi_quad: ycge_render_frame_ansi_quad's stream for those planes.  ycge_video_blit_ansi_quad_delta: the layered 24-bit
 *   delta contract with the glyph, as ycge_render_frame_ansi_quad_delta; layers are composed as there.  ycge_ansi_rgb_stream_bound stands.
 *   State.  One terminal per context: these streams and the frame quad streams share the quadrant family's delta state, as
 *   ycge_video_blit_ansi_delta shares ycge_render_frame_ansi_delta's - a video _quad_delta behind a frame _quad_delta of the same geometry key
 *   is a delta, and the other way round; a stream of another family in between makes the next one a keyframe.  min_contrast is not part of
 *   the key.  A blit changes nothing a traced frame reads, and first joins the frames in flight.
 *   Refused before any device work, nothing written then or later, the message naming the value, the context usable and the delta state
 *   untouched (YCGE_ERR_INVALID_ARG): everything the corresponding ycge_video_blit / _ansi_rgb / _ansi_rgb_delta call refuses; an odd or
 *   < 2 super_sample; min_contrast outside 0..255; all destinations NULL. */
int ycge_video_blit_quadrants(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                              float *out_top_bottom_sdr /* may be NULL */, float *out_quad_sdr /* fbW*fbH*12, may be NULL */,
                              uint16_t *out_glyphs /* fbW*fbH, may be NULL */, uint8_t *out_rgba /* fbW x 2 fbH RGBA8, may be NULL */,
                              int32_t min_contrast);
int ycge_video_blit_ansi_quad(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                              int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                              int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t min_contrast,
                              uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr /* may be NULL */);
int ycge_video_blit_ansi_quad_delta(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                                    int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                                    int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance,
                                    int32_t keyframe, int32_t min_contrast, uint8_t *out_stream, size_t capacity, size_t *out_len,
                                    uint32_t *out_info /* 4 words or NULL */, float *out_top_bottom_sdr /* may be NULL */);
/* --- The console's other framebuffers in the device streams: layers, any glyph.  Terminal registers a console-sized entity framebuffer
 * first (Renderer/Terminal.cs:53-55), RaytraceEntity adds its own on top (RaytraceEntity.cs:297-298), any entity may add more, and
 * ANSITerminalRenderer.GetChexelForPoint (:67-84) composes them: the topmost framebuffer whose chexel at the point has Char != ' ' wins,
 * else the default cell.  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing struct or prototype changes; a
 * host detects the export by symbol lookup.
 *   ycge_chexel: Chexel.Char as its UTF-16 code unit, ForegroundColor.color_f32, BackgroundColor.color_f32 (28 bytes; pad is ignored).
 *   ycge_console_layer: a Framebuffer - ViewportX, ViewportY, Width, Height - and its cells row by row: cell (x, y) at cells[y * w + x].
 *   ycge_console_set_layers: layers[0..n) are the console's OTHER framebuffers in frameBuffers order, bottom first; raytrace_at in 0..n says
 *   how many of them lie below the raytrace framebuffer, which keeps coming from the stream call's own viewport_x, viewport_y and the
 *   context's size.  From this call on every one of the eight stream calls of the context (ycge_render_frame_ansi, ycge_video_blit_ansi, their
 *   _delta, _rgb and _rgb_delta forms) writes the bytes Render() writes for that list:
 *     GetChexelForPoint taken literally - a layer cell with ch == ' ' is transparent whatever its colours; raytrace chexels are '▀' and
 *     opaque; ch == 0 is a character; nothing covering a point gives ' ' in the default colours.  Layers may hang off any edge of the console
 *     or lie wholly outside it.
 *     A cell's character is its code unit as AppendCharUtf8 (:204-224) writes it: 1 byte below 0x80, 2 below 0x800, else 3 - a lone surrogate
 *     in its 3-byte form.  No character is longer than '▀', so ycge_ansi_stream_bound and ycge_ansi_rgb_stream_bound stand as they are.
 *     A layer's colours are encoded once, by the encoder the frames use (the one behind ycge_render_frame_chexels, on the layer's colours as
 *     top / bottom): ansi(fg), ansi(bg) for the 256-colour streams, RGB8(fg), RGB8(bg) for the 24-bit ones.
 *   The call copies the cells (the host may reuse its arrays), costs the upload and encode of the layers' cells only, and joins frames in
 *   flight like every scene call.  n == 0 removes all layers: the streams are then byte for byte what they are without this call.  The layers
 *   survive ycge_resize and ycge_scene_upload.
 *   All or nothing: a refused call leaves the previous layers in force.  YCGE_ERR_INVALID_ARG, the message naming the value: n outside
 *   0..YCGE_CONSOLE_MAX_LAYERS, raytrace_at outside 0..n, a NULL layers with n > 0, a NULL cells, w or h <= 0, more than 2^26 cells over all
 *   layers; a peer context refuses as the stream calls do.
 *   The delta contract with layers in force (beside the rules at ycge_render_frame_ansi_delta and ycge_render_frame_ansi_rgb_delta):
 *     What the terminal shows is a console-wide composite of {character, colours}; prev / shown is the composite the last _delta stream left.
 *     changed(x, y) holds for ANY console cell whose character differs from what was last handed out, or whose colours differ - in 256
 *     colours either index, in 24-bit colour the largest channel difference exceeding tolerance.  emitted, run starts, the last-cell rule,
 *     merge_gap and out_info are as without layers; after a 24-bit delta shown = cur for every emitted cell, and its character always is cur's.
 *     A ycge_console_set_layers call that keeps n > 0 never forces a keyframe: moved, resized or edited layers resend only the cells whose
 *     composite changed.  Keyframes are the causes listed at the _delta calls, plus the first _delta call after the layers went from none
 *     to some or back. */
typedef struct ycge_chexel { uint16_t ch; uint16_t pad; float fg[3]; float bg[3]; } ycge_chexel;   /* 28 bytes */
typedef struct ycge_console_layer { int32_t x, y, w, h; const ycge_chexel *cells; } ycge_console_layer;
#define YCGE_CONSOLE_MAX_LAYERS 16
int ycge_console_set_layers(ycge_ctx *ctx, const ycge_console_layer *layers, int32_t n, int32_t raytrace_at);
/* --- Quadrant-glyph frames: 2 x 2 sub-cells a chexel, fitted on the device.  Every presenter above ends in '▀' with a top and a bottom
 * colour: two samples a console cell.  With an even super_sample the frame holds more, and the quadrant block glyphs (U+2596..U+259F, '▌',
 * '▀': all in the BMP, all 3 UTF-8 bytes) show a 2 x 2 grid in two colours.  The reference has no such presenter, so these rules define the
 * result; the tone map and LinearToSrgb8 are the frame's own.  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing
 * struct or prototype changes; a host detects the exports by symbol lookup.
 *   Sub-cell colours.  super_sample = ss must be even.  Chexel (cx, cy) covers hi-res columns cx ss .. cx ss + ss - 1 and rows 2 cy ss ..
 *   2 cy ss + 2 ss - 1 of the denoised buffer the tone map reads (YCGE_BUF_DENOISED).  Quadrant k - 0 = TL, 1 = TR, 2 = BL, 3 = BR - is ss / 2
 *   columns (the left / right half) by ss rows (the top / bottom half-cell's).  Its colour: the binary32 sum of its samples in row-major order
 *   (rows outer, columns inner, per channel, from 0), times 1.0f / (float)((ss / 2) ss), through the frame's MapPixel with the frame's effective
 *   exposure (stats.exposure), gamma 2.2, saturation 2.0, vibrance 0.  out_quad_sdr: fbW*fbH*12 f32, {TL rgb, TR rgb, BL rgb, BR rgb} a chexel.
 *   The fit, all integer from the bytes on, with min_contrast = M in 0..255:
 *     Q[k][c] = the sRGB8 byte ycge_render_frame_chexels' out_rgba holds for that colour (Clamp01, LinearToSrgb8).
 *     S0[c] = Q[0][c] + .. + Q[3][c], mean0[c] = (2 S0[c] + 4) / 8 (integer division).
 *     If the largest |Q[k][c] - mean0[c]| over k, c is <= M the mask is m = 0.  Otherwise, for m in 0..7 - bit 0 = TL, bit 1 = TR, bit 2 = BL
 *     in the foreground F, the rest and always BR the background B - score(m) = w(|B|) |S_B|^2 + (F empty ? 0 : w(|F|) |S_F|^2), w(1..4) =
 *     12, 6, 4, 3, |S|^2 the sum over channels of the squared channel sum (int32; below 2^24).  The largest score wins, ties to the smallest
 *     m: a minimiser of the squared error of the two-colour approximation.
 *     bg[c] = (2 S_B[c] + |B|) / (2 |B|), fg likewise over F; m = 0: fg = bg.
 *     The glyph by m: 0 U+2580 (fg == bg), 1 U+2598, 2 U+259D, 3 U+2580, 4 U+2596, 5 U+258C, 6 U+259E, 7 U+259B.  No cell is ever ' ': a
 *     raytrace cell stays opaque under GetChexelForPoint's rule.
 *     M is there so that the +-1 flicker TAA leaves in a resting picture does not flip masks, and with them glyphs, every frame.  Default 0.
 *   ycge_render_frame_quadrants: ycge_render_frame_chexels' frame - the same frame state, the same SDR array bit for bit - with
 *   out_quad_sdr; out_glyphs, fbW*fbH code units; out_rgba in exactly out_rgba's layout there (fbW x 2 fbH RGBA8, row 2 cy = fg, row 2 cy + 1
 *   = bg, alpha 255).  Any subset of the four destinations may be NULL, not all; pageable or page-locked as the chexel call handles them.
 *   ycge_render_frame_ansi_quad: ycge_render_frame_ansi_rgb's stream, rule for rule - clear prefix, per-row cursor move, the three-branch
 *   escape against the previous cell, the trailer ESC[0m - with a covered cell's character and triples the fitted glyph, fg, bg.  Uncovered
 *   cells are ' ' in the default colours.  ycge_ansi_rgb_stream_bound stands: every glyph is 3 bytes.
 *   ycge_render_frame_ansi_quad_delta: the layered 24-bit delta contract above (ycge_console_set_layers), layers or none: shown is a
 *   console-wide composite of {character, fg, bg}; changed(x, y) where the character differs or the largest channel difference exceeds
 *   tolerance; emitted cells, run starts, merge_gap, the last-cell rule, out_info and "shown = cur for every emitted cell, its character
 *   always cur's" as there.  A keyframe is the full quad stream, byte for byte.
 *   Layers.  With ycge_console_set_layers in force the fitted cells take the raytrace framebuffer's place in the composite - same order, same
 *   opacity; the other framebuffers behave as they do in the other streams.
 *   State.  One terminal per context: the quad family is a third beside the 256-colour and 24-bit ones.  A delta of one family is a keyframe
 *   after any stream of another, and every keyframe cause listed at ycge_render_frame_ansi_rgb_delta applies.  min_contrast is not part of
 *   the geometry key.  An argument refusal leaves the state untouched.
 *   Refused before any device work, nothing written then or later, the message naming the value (YCGE_ERR_INVALID_ARG): an odd super_sample;
 *   min_contrast outside 0..255; everything the corresponding _chexels / _ansi_rgb / _ansi_rgb_delta call refuses - all destinations NULL, a
 *   NULL stream or length, capacity below the bound, defaults outside 0..15, a peer context, RCCL with lean slabs, tolerance, merge_gap.
 *   Not offered: 256-colour and console-16 forms, frames in flight, sextants and octants, a temporal hysteresis beyond M. */
int ycge_render_frame_quadrants(ycge_ctx *ctx, float *out_top_bottom_sdr /* may be NULL */, float *out_quad_sdr /* fbW*fbH*12, may be NULL */,
                                uint16_t *out_glyphs /* fbW*fbH, may be NULL */, uint8_t *out_rgba /* fbW x 2 fbH RGBA8, may be NULL */,
                                int32_t min_contrast, ycge_frame_stats *stats);
int ycge_render_frame_ansi_quad(ycge_ctx *ctx, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                int32_t default_bg16, int32_t clear_screen, int32_t min_contrast, uint8_t *out_stream, size_t capacity,
                                size_t *out_len, float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_render_frame_ansi_quad_delta(ycge_ctx *ctx, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                      int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance, int32_t keyframe,
                                      int32_t min_contrast, uint8_t *out_stream, size_t capacity, size_t *out_len,
                                      uint32_t *out_info /* 4 words or NULL */, float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
/* --- Sixel frames: the traced picture per pixel, as a DEC sixel stream built on the device.  Every presenter above ends in a character cell:
 * '▀' shows two samples a cell, a quadrant glyph four in two colours, and the box average of the tone map removes the rest of what a frame
 * at super_sample > 1 traced.  A sixel stream (xterm, foot, WezTerm, Windows Terminal, iTerm2, Konsole, mlterm, tmux 3.4) shows every sample.
 * The reference has no such presenter, so these rules define the result.  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10,
 * no existing struct or prototype changes; a host detects the exports by symbol lookup.
 *   Geometry.  The picture is the hi-res buffer: W = fbW ss columns by H = 2 fbH ss rows, row 0 on top.  Any super_sample >= 1.
 *   Pixel colour.  Pixel (x, y) is the frame's MapPixel of sample (x, y) of the denoised buffer (YCGE_BUF_DENOISED) - no box sum - with the
 *   frame's effective exposure (stats.exposure), gamma 2.2, saturation 2.0, vibrance 0.  Its sRGB8 bytes are Clamp01 / LinearToSrgb8 of the three
 *   channels, from the threshold tables ycge_render_frame_chexels uses: at super_sample 1 the RGBA plane is that call's out_rgba plane, byte
 *   for byte.  The ordinary tone map still runs: the SDR array is ycge_render_frame's, bit for bit, and so is the frame state.
 *   Palette.  216 registers, a 6 x 6 x 6 cube: register i = 36 r + 6 g + b with levels r, g, b in 0..5 is defined in the stream as
 *   #i;2;20r;20g;20b (sixel percentages) and stands for the bytes 51 r, 51 g, 51 b.
 *   Quantiser.  Integer arithmetic on each byte v.  dither = 0: level = (v + 25) / 51, the nearest cube level.  dither = 1:
 *   level = (32 v + 102 D[y & 3][x & 3] + 51) / 1632 with the 4 x 4 Bayer matrix D = {0,8,2,10; 12,4,14,6; 3,11,1,9; 15,7,13,5} indexed by the
 *   hi-res pixel.  Both give 0..5 for every byte.
 *   Stream.  In this order: ESC[2J only if clear_screen is non-zero; ESC[<viewport_y + 1>;<viewport_x + 1>H; ESC P q; "1;1;<W>;<H>; the 216
 *   register definitions, ascending (3130 bytes, always the same); the bands; ESC \.  Band k holds rows 6 k .. 6 k + 5; rows at or past H
 *   contribute no bits.  Inside a band the colours present in it come in ascending register order.  Colour c gives one line: #<c>, then the
 *   line's sixels - sixel x has bit r set where pixel (x, 6 k + r) is c.  Every column after the last non-zero sixel is omitted; the rest is
 *   cut into maximal runs of equal sixels; a run of n >= 4 is written !<n> and the character 63 + bits, a run of n <= 3 the character n
 *   times; leading empty columns are runs of '?'.  Between two lines of a band stands '$', behind every band but the last '-'.
 *   Known answer.  The 5 x 7 picture with the register rows {0 0 0 0 215} {0 7 7 7 7} {0 7 7 7 7} {0 0 0 0 0} x 3 {43 43 43 43 0} at viewport
 *   (2, 1) with clear has the body #0~xxxw$#7?!4E$#215!4?@-#0!4?@$#43!4@ behind the register definitions, then ESC \: 3190 bytes in all.
 *   Bound.  ycge_sixel_stream_bound(W, H) = 3200 + ceil(H / 6) min(216, 6 W) (W + 5): a line is at most #ddd, W characters and a separator.
 *   It refuses (YCGE_ERR_INVALID_ARG) a geometry whose bound does not fit 32 bits.  capacity below the bound is refused before any device
 *   work, as the ANSI calls do; exactly *out_len bytes are written, no byte at or past them is touched.  The bound is generous - 74 MB for
 *   1920 x 1072 pixels against streams of a few hundred KB - and a pageable buffer of that size costs nothing it does not use: allocate it
 *   once, untouched pages are never backed.  More than 6 * 65535 rows are refused.
 *   ycge_render_frame_pixels: the planes.  out_rgba W x H RGBA8 (alpha 255), out_index W x H registers; any subset of the three destinations
 *   may be NULL, not all; pageable or page-locked as the chexel call handles them.  It leaves the ANSI delta state alone.
 *   ycge_render_frame_sixel: the stream of those registers.  The picture paints over the terminal's cells: after a successful call the
 *   context's ANSI delta state is invalid and the next _delta call of any family is a keyframe.  Layers set with ycge_console_set_layers
 *   are not composed into the picture: a host writes its text cells behind the image.
 *   ycge_sixel_encode_host: the same stream in plain C++ from a register plane (values 0..215), no context and no device - the yardstick
 *   of the kernels, and with YCGE_SIXEL_HOST=1 in the environment the encoder ycge_render_frame_sixel runs on the plane read back.
 *   Refused before any device work, nothing written, frame and delta state untouched, the message naming the value (YCGE_ERR_INVALID_ARG):
 *   a NULL stream or length; capacity below the bound; a negative viewport_x or viewport_y; dither outside 0..1; all destinations NULL (the
 *   planes call); whatever ycge_render_frame_chexels refuses - peer contexts, RCCL with lean slabs.
 *   Not offered: frames in flight; layers composed into the
 *   picture; a grey ramp; pixel replication to scale the image; the kitty graphics protocol (the out_rgba plane of
 *   ycge_render_frame_pixels is what a host would base64 for it). */
int ycge_sixel_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes);
int ycge_render_frame_pixels(ycge_ctx *ctx, float *out_top_bottom_sdr /* may be NULL */, uint8_t *out_rgba /* W x H RGBA8, may be NULL */,
                             uint8_t *out_index /* W*H registers, may be NULL */, int32_t dither, ycge_frame_stats *stats);
int ycge_render_frame_sixel(ycge_ctx *ctx, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t dither, uint8_t *out_stream,
                            size_t capacity, size_t *out_len, float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_sixel_encode_host(const uint8_t *index, int32_t px_w, int32_t px_h, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen,
                           uint8_t *out_stream, size_t capacity, size_t *out_len);
/* --- Sixel in Video mode, and delta sixel streams.  Added after ABI 10 without changing it, as the block above; found by symbol lookup.
 *   Video mode's pixel plane (ycge_video_blit_pixels).  Geometry: the blit's hi-res grid, W = fbW ss by H = 2 fbH ss, with the letterbox and
 *   the tables of ycge_video_blit.  Sample: pixel (x, y) is the per-channel Clamp01 of SampleSourceLanczos at hi-res sample (x, y) - the value
 *   ycge_video_blit adds into its half-cell sum - with no box sum and no tone map.  Bytes: its sRGB8 bytes from the threshold tables, alpha
 *   255.  Register: the sixel quantiser above, the Bayer matrix indexed by the hi-res pixel.  SDR: where out_top_bottom_sdr is asked for it is
 *   ycge_video_blit's, bit for bit.  At super_sample 1 out_rgba is ycge_video_blit's out_rgba, byte for byte.  Any subset of the three
 *   destinations may be NULL, not all.  The call leaves the frame state and the delta state alone.
 *   ycge_video_blit_sixel: the stream of that register plane; arguments, bound, refusals and bytes are ycge_render_frame_sixel's for the same
 *   plane, and ycge_video_blit's refusals of the source frame apply too.  The frame state stays untouched, as for every blit.
 *   Delta streams (ycge_render_frame_sixel_delta, ycge_video_blit_sixel_delta).  prev is the register plane of the last sixel stream this
 *   context handed out while its state is valid, cur this call's.  A KEYFRAME - the stream of ycge_render_frame_sixel (ycge_video_blit_sixel)
 *   for the same arguments, byte for byte - is returned when there is no valid prev, when {W, H, viewport_x, viewport_y} differ from prev's,
 *   when clear_screen != 0 or when keyframe != 0.  Else, for band k (rows 6 k .. 6 k + 5, cut at H), lo_k is the smallest column in which
 *   any of the band's rows differs between prev and cur and hi_k the largest such column + 1; the band is unchanged when there is none.
 *   The delta stream is, in this order: ESC[<viewport_y + 1>;<viewport_x + 1>H; ESC P 0;1 q (P2 = 1: a zero bit leaves its pixel as it is -
 *   the only difference from the full header); "1;1;<W>;<H>; the 216 register definitions; the body; ESC \.  The body: bands 0 .. the last
 *   changed band joined by '-', an unchanged band empty, nothing behind the last changed band, empty when no band changed.  A changed band has
 *   one line per register present in columns lo_k .. hi_k - 1 of the band in cur, ascending, joined by '$': #<c>, then sixel x with bit r set
 *   where lo_k <= x < hi_k and cur(x, 6 k + r) == c, every other sixel 0, written by the full stream's rules (leading empty columns are runs
 *   of '?', runs from 4 on !<n>, the empty tail omitted).  When every pixel of every column changed the body is the full stream's body.
 *   out_info (4 words or NULL): {keyframe returned, changed bands, pixels painted - span width x band rows, summed -, lines}; the three
 *   counts are 0 on a keyframe.
 *   Known answers.  prev the 5 x 7 picture above at viewport (2, 1): (2, 6) -> 0 and (3, 6) -> 7 gives the body -#0??@$#7???@, 3165 bytes,
 *   {0, 1, 2, 2}; (1, 1) -> 0 and (3, 2) -> 215 gives #0?zxx$#7?CEA$#215???C, 3174 bytes, {0, 1, 18, 3}; no change gives the empty body, 3152
 *   bytes, {0, 0, 0, 0}.
 *   Bound.  A delta never exceeds ycge_sixel_stream_bound, which stays the capacity to pass: the header is 3 bytes longer (and has no ESC[2J),
 *   a changed band's lines fit its budget as the full stream's do, and an unchanged band costs one byte out of a band budget of at least 36.
 *   State.  One terminal, one state a context: the sixel delta is one more family of the ANSI _delta calls' state, shared by frames and
 *   video.  prev advances only when one of the two delta calls returns YCGE_OK.  The next sixel delta is a keyframe after a failure behind the
 *   refusals, ycge_resize, a plain _sixel call of either mode, or any ANSI stream of any family; a sixel delta makes the next ANSI _delta
 *   call a keyframe.  The two planes calls leave the state alone, and a refusal of arguments leaves it as it was.
 *   Refusals: those of ycge_render_frame_sixel / ycge_video_blit_sixel, decided before any device work.
 *   ycge_sixel_encode_delta_host: the delta stream in plain C++ from the two planes (never a keyframe), the yardstick of the kernels and with
 *   YCGE_SIXEL_HOST=1 the encoder of the delta calls on the planes read back.
 *   Not offered: a tolerance or hysteresis, resending only the registers in use, frames in flight. */
int ycge_video_blit_pixels(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                           float *out_top_bottom_sdr /* may be NULL */, uint8_t *out_rgba /* W x H RGBA8, may be NULL */,
                           uint8_t *out_index /* W*H registers, may be NULL */, int32_t dither);
int ycge_video_blit_sixel(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t viewport_x, int32_t viewport_y,
                          int32_t clear_screen, int32_t dither, uint8_t *out_stream, size_t capacity, size_t *out_len,
                          float *out_top_bottom_sdr /* may be NULL */);
int ycge_render_frame_sixel_delta(ycge_ctx *ctx, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t keyframe, int32_t dither,
                                  uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info /* 4 words or NULL */,
                                  float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_video_blit_sixel_delta(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t viewport_x,
                                int32_t viewport_y, int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream, size_t capacity,
                                size_t *out_len, uint32_t *out_info /* 4 words or NULL */, float *out_top_bottom_sdr /* may be NULL */);
int ycge_sixel_encode_delta_host(const uint8_t *prev_index, const uint8_t *index, int32_t px_w, int32_t px_h, int32_t viewport_x, int32_t viewport_y,
                                 uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info /* 4 words or NULL */);
/* --- Adaptive sixel palette: median-cut registers built on the device, a second palette for the sixel streams of frames and Video mode.  The
 * cube's levels are 51 apart and need the ordered dither to hide their banding; these registers are cut from the picture at hand.  Added
 * after ABI 10 without changing it, as the blocks above; found by symbol lookup.  No cube call, struct or stream byte changes.  The reference
 * has no such presenter, so these rules define the result.  Everything is integer arithmetic on the RGBA8 plane of ycge_render_frame_pixels
 * (ycge_video_blit_pixels), W x H pixels.
 *   Bins.  Pixel bytes (r, g, b) fall in bin (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3): 32 768 bins with coordinates 0..31 on three axes.
 *   A bin holds its pixel count and the three sums of the actual bytes, all uint32: W * H > 2^24 is refused so that the sums fit.
 *   Boxes.  Boxes partition the whole 32^3 bin cube, empty bins included.  Start with box 0, the whole cube, n = 1.  Eight passes; a pass looks
 *   at the boxes 0 .. n0 - 1 that exist at its start, in index order.  For box b the occupied extent on an axis is the largest minus the
 *   smallest coordinate among the box's bins with a count above zero; axis a is the one with the largest extent, ties to the first of r, g,
 *   b; the box splits if that extent is at least 1.  With omin, omax its occupied bounds on a, m[t] the pixel count at coordinate t and total
 *   their sum, the cut c is the smallest t in omin .. omax - 1 with 2 (m[omin] + .. + m[t]) >= total, or omax - 1 if there is none.  Bins of
 *   the box with coordinate <= c stay box b, the others become box n0 + rank, rank the number of boxes below b that split in this pass.
 *   After the pass n = n0 + the number of splits; both halves hold pixels.  After eight passes n <= 256 is the number of registers.
 *   Register colour.  Box i with pixel count k and byte sums S has the bytes m = (2 S + k) / (2 k) per channel and the sixel percentages
 *   (200 m + 255) / 510; it is defined in the stream as #i;2;pr;pg;pb in canonical decimal.  Only registers 0 .. n - 1 are defined, ascending.
 *   Register plane.  index(x, y) = the box of the pixel's bin.
 *   Stream.  ycge_render_frame_sixel's, rule for rule - ESC[2J where asked, the cursor, ESC P q, the raster attributes, the bands, their lines in
 *   ascending register order, the runs, ESC \ - with these register definitions in place of the cube's 216.
 *   Known answer.  The 6 x 12 picture whose rows 0..5 are (0, 0, 0) and rows 6..11 (255, 255, 255), at viewport (0, 0) without clear:
 *   ESC[1;1H ESC P q "1;1;6;12 #0;2;0;0;0#1;2;100;100;100 #0!6~-#1!6~ ESC \ (without the spaces).
 *   Bound.  ycge_sixel_palette_stream_bound(W, H) = 4700 + ceil(H / 6) min(256, 6 W) (W + 5): 256 definitions of at most 18 bytes are 4608
 *   bytes and the prefix keeps the 70 bytes of slack the cube's 3200 has over its 3130; a line is still #ddd, W characters and a separator.
 *   Its refusals are ycge_sixel_stream_bound's.
 *   Hold.  hold = 0 builds the palette from this call's picture and keeps it in the context: the bin-to-box table, the register definitions
 *   and n.  hold = 1 maps this picture through the kept palette and skips the build - every bin has a box, so the map is total, and the
 *   colours of a picture at rest do not shimmer with TAA's +-1; with no kept palette hold = 1 builds one.  The palette is independent of
 *   geometry: ycge_resize keeps it, frames and video share it (as they share the delta state), the hooks of ycge_hooks.h read and replace it
 *   too.  A failure behind the refusals drops it.
 *   State.  A stream call paints over the cells and over the cube's picture: it invalidates the context's delta state exactly as a plain
 *   _sixel call does.  The two planes calls leave the delta state alone.
 *   ycge_render_frame_sixel_palette / ycge_video_blit_sixel_palette: the stream; out_palette 256 x RGBA8 of the bytes m (alpha 255, unused
 *   entries zero) and out_count n, either may be NULL.  The SDR and the frame state are ycge_render_frame's (ycge_video_blit's), bit for bit.
 *   ycge_render_frame_pixels_palette / ycge_video_blit_pixels_palette: the planes.  out_rgba is the cube calls' plane, out_index holds the
 *   adaptive registers, the palette and count come with it; any subset of the destinations may be NULL, not all.
 *   ycge_sixel_palette_host (out_pct: 256 x 3 percentages, unused entries zero; any output may be NULL, not all) and
 *   ycge_sixel_encode_palette_host (registers below count, count 1..256, percentages 0..100): the rule and the stream in plain C++, no
 *   context and no device - the kernels' yardstick, and with YCGE_SIXEL_HOST=1 what the stream calls run on the RGBA plane read back.
 *   Refusals: those of the cube calls - decided before any device work, nothing written, the frame state, the delta state and the kept
 *   palette as they were, the message naming the value - plus hold outside 0..1 and W * H > 2^24.
 *   Not offered: a dither parameter (the point of the palette is not to need one); the delta form under an adaptive palette (registers
 *   change meaning between builds, so the diff would have to compare colours); a grey ramp; frames in flight. */
int ycge_sixel_palette_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes);
int ycge_render_frame_sixel_palette(ycge_ctx *ctx, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t hold, uint8_t *out_stream,
                                    size_t capacity, size_t *out_len, uint8_t *out_palette /* 256 x RGBA8, may be NULL */,
                                    int32_t *out_count /* may be NULL */, float *out_top_bottom_sdr /* may be NULL */, ycge_frame_stats *stats);
int ycge_video_blit_sixel_palette(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t viewport_x,
                                  int32_t viewport_y, int32_t clear_screen, int32_t hold, uint8_t *out_stream, size_t capacity, size_t *out_len,
                                  uint8_t *out_palette /* 256 x RGBA8, may be NULL */, int32_t *out_count /* may be NULL */,
                                  float *out_top_bottom_sdr /* may be NULL */);
int ycge_render_frame_pixels_palette(ycge_ctx *ctx, float *out_top_bottom_sdr /* may be NULL */, uint8_t *out_rgba /* W x H RGBA8, may be NULL */,
                                     uint8_t *out_index /* W*H registers, may be NULL */, int32_t hold, uint8_t *out_palette /* 256 x RGBA8, may be NULL */,
                                     int32_t *out_count /* may be NULL */, ycge_frame_stats *stats);
int ycge_video_blit_pixels_palette(ycge_ctx *ctx, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel,
                                   float *out_top_bottom_sdr /* may be NULL */, uint8_t *out_rgba /* W x H RGBA8, may be NULL */,
                                   uint8_t *out_index /* W*H registers, may be NULL */, int32_t hold, uint8_t *out_palette /* 256 x RGBA8, may be NULL */,
                                   int32_t *out_count /* may be NULL */);
int ycge_sixel_palette_host(const uint8_t *rgba, int32_t px_w, int32_t px_h, uint8_t *out_index, uint8_t *out_palette /* 256 x RGBA8 */,
                            uint8_t *out_pct /* 256 x 3 */, int32_t *out_count);
int ycge_sixel_encode_palette_host(const uint8_t *index, const uint8_t *pct /* count x 3 */, int32_t count, int32_t px_w, int32_t px_h, int32_t viewport_x,
                                   int32_t viewport_y, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len);
/* --- ANSI streams with frames in flight: the four frame forms above - ycge_render_frame_ansi, _ansi_delta, _ansi_rgb, _ansi_rgb_delta - queued
 * as ycge_render_frame_async_sdr queues a frame.  The synchronous calls read the stream's length on the host and copy exactly that many
 * bytes, which takes a synchronisation inside the call; here a kernel behind the stream's kernels (k_ansi_deliver, csrc/ycge_ansi_flight.hip)
 * copies exactly `length` bytes into the caller's page-locked buffer and fills the caller's record, and the call returns at once.  Added
 * after ABI 10 without changing it: YCGE_ABI_VERSION stays 10; a host detects the export by symbol lookup.  Video blits stay synchronous.
 *   req: the console, viewport, defaults and clear_screen of the synchronous calls; rgb picks the colour form, delta the stream; merge_gap,
 *   tolerance and keyframe are the _delta calls' (tolerance the 24-bit one's) and must be 0 where the form does not read them.
 *   Bytes.  The bytes, the length and info are those the synchronous export of the same form would have returned, for the same sequence of
 *   calls on the same context, frame for frame; layers in force are included.  Exactly `length` bytes of out_stream are written, never a
 *   byte at or past them.  The frame state and the optional SDR are ycge_render_frame_async_sdr's.
 *   When.  out_stream, out_result and the SDR array are the caller's to read after ycge_wait, or any other call on the context - they all
 *   join first.  There is no polling contract.  A caller with several frames in flight passes a buffer and a record per frame.
 *   Delta state.  A queued call counts as handed out when it is queued: the keyframe decision and the flip of the held planes happen then,
 *   and the rules at the _delta calls hold with "call" read as "queued call".  A synchronous delta behind queued deltas is a delta against
 *   the last queued frame.  A call that fails behind its argument checks makes the next one a keyframe; a call refused for its arguments
 *   leaves the state untouched.  The host writes the streams whole and in queue order.
 *   Refused with YCGE_ERR_INVALID_ARG, the message naming the parameter or value, nothing written then or later: a NULL req, out_stream or
 *   out_result; out_stream not page-locked over all of [out_stream, out_stream + capacity) or not 16-byte aligned; out_result not page-locked
 *   or not 8-byte aligned; an SDR array that is not page-locked; capacity below the form's bound; merge_gap outside 0..8, tolerance outside
 *   0..255; non-zero delta fields on a full stream, a tolerance without rgb; a console that is not positive or whose bound reaches 2^32,
 *   defaults outside 0..15; and whatever the other frames in flight refuse - peer and multi-device contexts, config.capture_debug,
 *   config.count_work, the RCCL exchange with lean slabs.
 *   status.  0; or 1: the device stream exceeded `capacity` (the capacity check above makes that a fault of the library), nothing was copied.
 *   The call that joins such a frame - ycge_wait or any other - fails once with YCGE_ERR_DEVICE, and the next delta is a keyframe. */
typedef struct ycge_ansi_async {      /* 48 bytes */
    int32_t console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen;
    int32_t rgb;        /* 0: 38;5 / 48;5 indices, 1: 24-bit triples */
    int32_t delta;      /* 0: the full stream, 1: the delta stream */
    int32_t merge_gap, tolerance, keyframe;   /* delta only; tolerance with rgb only; otherwise must be 0 */
} ycge_ansi_async;
typedef struct ycge_ansi_async_result {   /* 32 bytes, page-locked, 8-byte aligned */
    uint64_t length;
    uint32_t info[4];   /* {keyframe returned, changed, emitted, run starts}; a full stream: {1, 0, 0, 0} */
    uint32_t status;    /* 0, or 1: the device stream exceeded capacity, nothing was copied */
    uint32_t reserved;
} ycge_ansi_async_result;
int ycge_render_frame_async_ansi(ycge_ctx *ctx, const ycge_ansi_async *req, uint8_t *out_stream, size_t capacity,
                                 ycge_ansi_async_result *out_result, float *out_top_bottom_sdr /* may be NULL */);
/* --- OBJ meshes from file bytes: MeshLoader.FromObj (RayTracing/MeshLoader.cs:12-149) up to the float soup ycge_mesh.triangles takes, parsed
 * on the device.  Added after ABI 10 without changing it (YCGE_ABI_VERSION stays 10, no struct changes; detect by symbol lookup).
 *   The contract, byte by byte ("the reference's loader" restated correctly; tests/obj_restatement.py is its yardstick):
 *   Lines    StreamReader.ReadLine: a line ends at \n, \r\n or a lone \r, the last one needs no terminator; a UTF-8 byte-order mark at
 *            offset 0 is skipped; lines count from 1.  An empty line or one whose first byte is '#' is skipped (" # x" is not).
 *   Tokens   split at char.IsWhiteSpace: in ASCII, inside a line, space, \t, \v, \f - 0x1C..0x1F are not separators.
 *   v lines  first token exactly v and at least 4 tokens: tokens 1..3 are parsed, the rest never looked at; fewer tokens add nothing.
 *   f lines  first token exactly f and at least 4 tokens: every token is cut at its first '/' and read by ParseIndex - empty gives 0,
 *            i > 0 gives i - 1, else count + i with count the positions read so far at this line - and a fan of tokens - 3 triangles
 *            (v0, v[k-1], v[k]) is added.  An index may name a vertex a later line defines: 0 <= index < the final count is checked last.
 *   Floats   [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?, correctly rounded to binary32 (nearest, ties to even; -0 stays
 *            -0; overflow gives +-inf, underflow a subnormal or zero) as .NET's float.Parse rounds - not by way of binary64.  Thousands
 *            separators, Infinity, NaN and surrounding blanks are refused.  Integers: [+-]? digits within int32.
 *   Refused  with YCGE_ERR_INVALID_ARG and a message, nothing held, the context usable - in this order: a NULL or empty text, 2^31 bytes
 *            or more; the first line in file order with a malformed float or integer token or (YCGE_ERR_UNSUPPORTED: it would need
 *            .NET's Unicode separators) a byte >= 0x80 outside a comment - the message names the 1-based line; more than 2^28 triangles;
 *            no position or no triangle (InvalidDataException); an index out of range - the message names the lowest triangle, counted
 *            from 0 in file order.
 *   Tail     (MeshLoader.cs:57-96, 107-148; binary32 operation by operation, no contraction) the box over the vertices any face uses;
 *            c = (min + max) * 0.5f; maxExtent by the three compares, 1 if <= 0; s = target_size / maxExtent; every vertex becomes
 *            (p - c) * s (skipped, as there, when a bound is infinite); then p * scale + t only when scale != 1 or t != 0; triangles are
 *            gathered in face order; the bounds are min / max over their corners.  Extremes do not depend on order except for the sign
 *            of a zero extreme, which in the reference follows HashSet enumeration order: here -0 orders below +0.  NaN is never an extreme.
 * ycge_obj_parse_host is pure host code - no context, no device: the yardstick and the fallback.  positions (3 * n_positions floats) and
 *   faces (3 * n_triangles int32) may be NULL (counts only); msg (may be NULL) receives the refusal's text, cut to msg_bytes.
 * ycge_obj_parse reads the text on the device and HOLDS the result in the context - one parsed OBJ at a time: the next parse,
 *   ycge_obj_release or ycge_destroy lets go of it.  No scene needed, none touched; frame counter, TAA history, exposure, schedule and
 *   statistics stay as they are.  It first waits for the frames in flight.  Pageable text goes up through page-locked staging of the
 *   library, page-locked text directly.  A peer context of the one-process multi-device form is refused; the root parses on devices[0].
 *   The host parser takes the whole file instead, with the same results and refusals, when the context was created with YCGE_OBJ_HOST in
 *   the environment, when the file has fewer than YCGE_OBJ_DEVICE_MIN bytes (default 0: the crossover is not yet measured), or when the
 *   kernels decline it: a float token outside their exact domain (more than 15 significant digits, or a decimal exponent beyond +-22 once
 *   the fraction digits are counted in), a line that is no comment longer than 1024 bytes.  info->on_device says who parsed.
 * ycge_obj_read copies the held positions / faces out (either may be NULL); MeshScenes.TryReadObjBoundsNormalized's union-find tail no
 *   longer needs them: ycge_obj_ground, below, runs it on the device.  ycge_obj_triangles is the tail above for the held OBJ, any number
 *   of times: out_triangles 9 * n_triangles floats, out_bounds (may be NULL) min xyz, max xyz; translate NULL = (0, 0, 0).  Both and
 *   ycge_obj_release without a held OBJ: YCGE_ERR_INVALID_ARG (release of nothing: YCGE_OK). */
typedef struct ycge_obj_info {
    int32_t n_positions, n_triangles;
    int64_t n_lines;
    int32_t on_device;           /* 1: the kernels parsed; 0: the host parser did */
    int32_t reserved;
} ycge_obj_info;
int ycge_obj_parse_host(const uint8_t *text, size_t bytes, float *positions, int32_t *faces, ycge_obj_info *info, char *msg, size_t msg_bytes);
int ycge_obj_parse(ycge_ctx *ctx, const uint8_t *text, size_t bytes, ycge_obj_info *info);
int ycge_obj_read(ycge_ctx *ctx, float *positions /* or NULL */, int32_t *faces /* or NULL */);
int ycge_obj_triangles(ycge_ctx *ctx, int32_t normalize, float target_size, float scale, const float translate[3], float *out_triangles, float out_bounds[6]);
int ycge_obj_release(ycge_ctx *ctx);
/* --- MeshScenes.AddMeshAutoGround (Scenes/MeshScenes.cs:173-184) on the held OBJ: what TryReadObjBoundsNormalized (:233-330) does behind its
 * parse - every mesh scene of the reference goes through it - and the placed triangles, with no geometry coming back before them.  Added
 * after ABI 10 without changing it (detect by symbol lookup).  The contract, bit for bit (tests/obj_ground_restatement.py is its yardstick):
 *   Components  vertices are joined by the edges (a, b) and (b, c) of every face; vertices no face names do not matter.
 *   The chosen  component: the one with the most faces; among equal counts the one whose first face comes first in file order (the
 *               reference's Dictionary enumerates in insertion order and compares with a strict >).  NOT the one with the lowest vertex.
 *   Centroid    cx = 0; for the kept faces in file order cx += ((A.x + B.x) + C.x) * (1 / 3f), every operation a rounded binary32 one, the
 *               product rounded before it is added; then cx *= 1 / (float)kept_faces.  y, z alike.  The order of the sum is part of the result.
 *   Bounds      over the vertices of the kept faces, of pos - centroid; min / max start at +inf / -inf, NaN never replaces an extreme, and
 *               -0 orders below +0 (as in ycge_obj_triangles' bounds; the reference's sign of a zero extreme follows HashSet order and
 *               cannot reach AddMeshAutoGround's result).
 *   Normalise   extent = rx; if (ry > extent) extent = ry; if (rz > extent) extent = rz; if (extent <= 0) extent = 1; s = 1 / extent;
 *               min = rMin * s, max = rMax * s.  A NaN extent passes every compare and stays NaN; infinite positions (the host parser's
 *               1e39) flow through as plain binary32 arithmetic.
 *   Placement   yTranslate = (target.y - min.y * scale) + 0.01f; then ycge_obj_triangles with normalize = 1, target_size = 1, scale and
 *               translate = (target.x, yTranslate, target.z).
 * ycge_obj_ground_host is pure host code - no context, no device: the yardstick and the fallback.  NULL arrays, counts <= 0 and an index
 *   out of range: YCGE_ERR_INVALID_ARG.
 * ycge_obj_ground works on the held OBJ, any number of times, with the same answer each time; towards frames in flight, peer contexts and
 *   a missing OBJ it behaves as ycge_obj_triangles does, and it touches nothing a frame reads.  The kernels (csrc/ycge_obj_ground.hip)
 *   label the components with a lock-free union-find, count faces per component, write one centroid term per face and add them in file
 *   order with one lane per axis; info->on_device says who ran the tail.  The host tail runs instead (on the held arrays, read back) when
 *   YCGE_OBJ_GROUND_HOST is set, for OBJs of fewer triangles than YCGE_OBJ_GROUND_DEVICE_MIN (both read once, at ycge_create), and
 *   when a kernel passes one of its loop bounds.
 * ycge_obj_triangles_auto_ground does all of it in one call: out_triangles 9 * n_triangles floats, out_bounds (may be NULL) min xyz, max
 *   xyz of the placed triangles, out_info (may be NULL) what ycge_obj_ground found. */
typedef struct ycge_obj_ground_info {      /* 64 bytes */
    float min[3], max[3];                  /* TryReadObjBoundsNormalized's out min / max */
    float centroid[3];                     /* cx, cy, cz after *= invT */
    float extent;                          /* after the <= 0 rule */
    int32_t n_components;                  /* components that own at least one face */
    int32_t component_faces, component_vertices, first_face;   /* of the chosen one */
    int32_t on_device, reserved;           /* 1: the kernels ran the tail; 0: the host tail did */
} ycge_obj_ground_info;
int ycge_obj_ground_host(const float *positions, int32_t n_positions, const int32_t *faces, int32_t n_triangles, ycge_obj_ground_info *out);
int ycge_obj_ground(ycge_ctx *ctx, ycge_obj_ground_info *out);
int ycge_obj_triangles_auto_ground(ycge_ctx *ctx, float scale, const float target[3], float *out_triangles, float out_bounds[6], ycge_obj_ground_info *out_info /* or NULL */);
int ycge_wait(ycge_ctx *ctx);
/* measurement: durations (ms) of the trace launches of the frames queued since the last call, oldest first (at most the last 1024);
 * waits for the frames in flight */
int ycge_async_trace_times(ycge_ctx *ctx, float *ms_out, int32_t capacity, int32_t *n_out);

/* What the frames-in-flight machinery of this context does (it decides timing only, never a pixel - a host or a benchmark reports it
 * beside its numbers).  The placed-value gate - "a trace starts when the trace before it has placed its last workgroup" - rests on an
 * OBSERVED property of the dispatcher (workgroups are placed in index order, so the last index is the last placed); where signal memory
 * or hipStreamWaitValue32 is not available the gate switches itself off and says so here. */
typedef struct ycge_flight_info {
    int32_t two_trace_streams;   /* consecutive frames in flight alternate between two trace streams                               */
    int32_t placed_gate;         /* 1: the placed-value gate is armed; 0: off (YCGE_FLIGHT_PLACED_GATE=0, no signal memory, ...) */
    int32_t post_gate;           /* a trace waits until the post stage before it has placed its persistent launch                */
    int32_t post_pair;           /* the post stages of consecutive frames run side by side                                      */
    int32_t frames_outstanding;  /* 1: frames in flight have not been joined yet                                                 */
    int32_t stage_pipeline;      /* 1: this scene's frames are traced by the stage kernels (k_wf_*), 0: by the single launch      */
    uint64_t placed_waits;       /* traces that were queued behind a placed value since the context was created                 */
} ycge_flight_info;
int ycge_flight_query(ycge_ctx *ctx, ycge_flight_info *out);
/* which exchange the one-process multi-device frame uses: *mode_out = YCGE_EXCHANGE_PEER_PUSH or YCGE_EXCHANGE_RCCL (the latter only when
 * config.multi_device_exchange asked for it AND librccl.so was found and its communicators came up); *world_out = devices that trace */
int ycge_exchange_query(ycge_ctx *ctx, int32_t *mode_out, int32_t *world_out);

/* --- multi-GPU halves of a frame (one process per GPU; the exchange between
 * them is one all-gather of the tile slabs, done by the caller with RCCL).
 * slab layout: for each owned tile in ascending tile_id, for each of its
 * 32x8 pixels in row-major order: 11 f32 {hdr rgb, albedo rgb, normal xyz,
 * depth, sky(0/1)}; ycge_tile_slab_bytes = padded per-rank size (equal on
 * all ranks so that a plain all-gather applies). */
int ycge_tile_slab_bytes(const ycge_ctx *ctx, size_t *bytes);
/* steps 1-4 of TryFlipAndBlit on this rank's tiles; d_slab = DEVICE pointer */
int ycge_trace_tiles(ycge_ctx *ctx, void *d_slab, void *hip_stream, ycge_frame_stats *stats);
/* un-permute world_size gathered slabs (DEVICE pointer, rank-major) into the
 * full-frame buffers, then steps 5-9 (TAA ... tonemap) on the full frame */
int ycge_resolve_gathered(ycge_ctx *ctx, const void *d_all_slabs, void *hip_stream,
                          float *out_top_bottom_sdr, ycge_frame_stats *stats);

/* --- the tile-RESIDENT form of the same partition (one process per GPU): TAA runs on every rank's OWN tiles and its history never
 * leaves the rank.  TemporalBlendWithClamp reads a 3x3 window (clampRadius = 1, RaytraceRenderer.cs:218), so a rank needs {hdr, sky}
 * of the one-pixel ring around each of its tiles from the ranks that own those pixels: one small all-to-all of halo records (4 floats
 * each: 1.3 KB per tile instead of the 8-11 KB of its slab), then TAA, then - for whoever shows the frame - a gather of the RESOLVED
 * history, 12 bytes per pixel.  Per frame and rank at 1920x1080 on 8 ranks: ~1.4 MB of halo records each way + 3.1 MB of history out,
 * against 8.3 MB out / 66 MB in for the all-gather of lean slabs.  The frame ends with TAA (no G-buffer on the consumer: the post stage
 * needs ycge_resolve_gathered).  K = config.tile_ring frame sets: K traces may be in flight, a trace waits for the resolve of frame
 * N - K.  Same pixels as the single-device frame, bit for bit (the halo records are copies, the per-pixel arithmetic is k_taa's).
 *
 *   every frame, every rank:   ycge_trace_tiles_resident(ctx, d_send, stream)        trace + gather of the records other ranks need
 *                              all_to_all(d_recv <- d_send) with ycge_halo_counts' split sizes (records of 4 floats)
 *                              ycge_resolve_tiles_resident(ctx, d_recv, d_hist_slab, stream)   ONE launch: TAA on own tiles with the halo taps read from
 *                                                                                 d_recv where the exchange left them, history slab
 *   the consumer:              all_gather / gather of the history slabs -> ycge_unpack_history(ctx, d_all_hist_slabs, stream) */
int ycge_halo_counts(ycge_ctx *ctx, int64_t *send_counts /* [world_size] */, int64_t *recv_counts /* [world_size] */);
int ycge_history_slab_bytes(const ycge_ctx *ctx, size_t *bytes);      /* padded per-rank size: equal on all ranks */
int ycge_trace_tiles_resident(ycge_ctx *ctx, void *d_halo_send, void *hip_stream, ycge_frame_stats *stats);
/* n (1..8, <= the free sets of the ring) CONSECUTIVE frames of this rank's tiles in ONE launch - for a caller that knows the next n camera
 * poses (a recorder, a benchmark, a render thread that runs ahead): poses = n x {pos x y z, yaw, pitch, fov_deg}, as n ycge_set_camera
 * calls would give them (the last stays the context's camera); d_halo_send = n buffers, filled as by n ycge_trace_tiles_resident calls.
 * A rank's share of ONE frame is a few thousand blocks whose longest chains leave most of the machine idle; n frames' blocks in one
 * launch are the work of a rank of world_size / n ranks - throughput approaches N-fold on N GPUs as n approaches N, at n frames of
 * latency.  The frames are then exchanged and resolved one by one, oldest first, as after n single calls; same pixels. */
int ycge_trace_tiles_resident_batch(ycge_ctx *ctx, int32_t n, const float *poses /* n x 6 */, void *const *d_halo_send /* n */, void *hip_stream);
int ycge_resolve_tiles_resident(ycge_ctx *ctx, const void *d_halo_recv, void *d_history_slab /* may be NULL */, void *hip_stream, ycge_frame_stats *stats);
int ycge_unpack_history(ycge_ctx *ctx, const void *d_all_history_slabs, void *hip_stream);

/* A live texture's next frame (what IFrameReader.GetCurrentFramePtr() will return while the coming frames are traced): bytes =
 * width * height * frame_bytes_per_pixel of texture `texture_index` of the last ycge_scene_upload.  The host sets
 * ycge_scene.has_dynamic_textures for such scenes (Scene.cs:30), which restarts the TAA history every frame. */
int ycge_scene_update_texture(ycge_ctx *ctx, int32_t texture_index, const uint8_t *frame, size_t bytes);

/* --- scene queries (ABI 10): the other caller of Scene.Hit in the reference, VolumeScene's camera physics (ground fan, collision
 * capsule, push-out: Scenes/VolumeScenes.cs), against the scene of the last successful ycge_scene_upload / ycge_scene_update_objects.
 * A query runs on a stream of its own: it waits for the device work of the last scene change and NOT for frames in flight (a query
 * between two ycge_render_frame_async calls leaves them in flight), and it changes nothing a frame reads - frame counter, TAA and exposure
 * state, trace outputs, schedule, timing and statistics.  It returns with the results in the caller's arrays.
 * Refused with YCGE_ERR_INVALID_ARG (ycge_last_error names the first bad ray; the output arrays are then unspecified): n < 0, a NULL
 * array when n > 0, a peer context of the one-process multi-device form, a ray with a NaN or inf in its origin, direction or tmin or a NaN
 * tmax, a ray whose binary32 dx*dx + dy*dy + dz*dz is not finite and > 0.  tmax = +inf, tmax = FLT_MAX and tmin > tmax (a miss) are
 * accepted.  YCGE_ERR_NO_SCENE before the first upload.  n = 0 with a scene: YCGE_OK. */
/* Scene.Hit (Scene.cs:71-75) for n rays against the scene of the last successful upload / update_objects.
 * rays: n x 8 f32 {ox, oy, oz, dx, dy, dz, tmin, tmax}; the direction is normalised as new Ray(o, d) does (Ray.cs:8-12,
 * Vec3.Normalized) and t is in units of the normalised direction.  Queries behave as screenU = screenV = 0.
 * hits: n x 10 f32 {t, p xyz, n xyz, albedo rgb} (HitRecord.T/P/N and Mat.Albedo as the hit leaves them - no texture sampling);
 * ids:  n x 2 i32 {Scene.Objects index, sub} with sub as YCGE_BUF_SUB_ID defines it; a miss is {-1, -1} and ten zeros. */
int ycge_scene_hit(ycge_ctx *ctx, const float *rays, int32_t n, float *hits, int32_t *ids);
/* Scene.Occluded / the boolean of Scene.Hit: occluded[i] = 1 when Scene.Hit(ray i, tmin, tmax) would return true, else 0. */
int ycge_scene_occluded(ycge_ctx *ctx, const float *rays, int32_t n, uint8_t *occluded);

/* --- VolumeScene's camera physics as one call a tick (Scenes/VolumeScenes.cs:51-159 Update, :165-530 HandleInput's moves and the helpers;
 * kernel k_camera_tick in csrc/ycge_camera.hip, the stepper csrc/ycge_camera_physics.h).  Added after ABI 10 without changing it:
 * YCGE_ABI_VERSION stays 10, no existing struct changes; a host detects the export by symbol lookup.
 * The reference's Update and HandleInput are a serial chain of Scene.Hit calls, most of which depend on the one before; through
 * ycge_scene_hit every one of them is a launch, three copies and a stream synchronise.  Here the chain's control runs on the device: one
 * launch, one small read-back and one synchronise a tick, and the body that comes back is the reference's, bit for bit.
 *   body   what VolumeScene keeps between ticks: CameraPos, verticalVelocity, shiftHoldTimer, repelVel, autoPlaced, isGrounded (in, out).
 *   world  WorldConfig's WorldHeight, WaterLevel and VoxelSize.Y.  EyeHeight ... RepelDamping (:20-39) are the library's.
 *   moves  one HandleInput call's effect on the body each, in the order the host received them, applied before the update:
 *            YCGE_CAMERA_MOVE_HORIZONTAL  AttemptMoveHorizontal(new Vec3(a, 0, b)): a, b = x and z of forwardXZ * (moveSpeed * dt) (:198-201)
 *            YCGE_CAMERA_MOVE_VERTICAL    AttemptMoveVertical(a), a widened to double (:204-205)
 *            YCGE_CAMERA_MOVE_JUMP        :208-212 - taken only when the body is grounded and `shift` is 0
 *            YCGE_CAMERA_MOVE_SHIFT       shiftHoldTimer = 0.15f (:177); a key with Shift held is this move, then the key's own
 *   then, when run_update != 0, Update's physics with delta_time_ms: ResolveIfEmbedded, the one-time auto placement with its early
 *   return, the shift timer, gravity and the two ground fans, ApplyWallRepulsion(dt), the fail-safe at y < -10.  LoadChunksAround and
 *   base.Update stay the host's.
 *   info   (may be NULL) what happened: rays_committed - the Scene.Hit calls of the serial order; rays_walked >= rays_committed - the rays the
 *          device walked, a window of consecutive rays side by side, those behind a ray that changed the state dropped and asked again;
 *          windows; micro-steps of the moves, micro-steps that ended a move blocked, slides, push-outs, embedded resolutions, ground
 *          snaps, auto placements, fail-safes.
 * The scene is the one of the last successful upload, update_objects, attach or edit, under ycge_scene_hit's contract: the tick runs on the
 * query stream, waits for the device work of the last scene change and NOT for frames in flight, and changes nothing a frame reads.
 * YCGE_ERR_NO_SCENE before the first upload.  Refused before any device work with YCGE_ERR_INVALID_ARG, *body untouched, the message
 * naming the move: a peer context, NULL body or world, n_moves outside 0..YCGE_CAMERA_MAX_MOVES, NULL moves with n_moves > 0, a
 * non-finite field, a move longer than YCGE_CAMERA_MAX_MOVE_LENGTH, an unknown kind.
 * Bounded: the reference's AttemptMoveHorizontal adds a slide's residual back to what remains (:275) and has no bound; here a move takes at
 * most YCGE_CAMERA_MAX_MICRO_STEPS micro-steps.  A tick that reaches that cap, or whose position stops being finite, returns
 * YCGE_ERR_UNSUPPORTED with *body and *info unchanged; the message says which cap and which move.  *body and *info are written on success
 * only.  YCGE_CAMERA_HOST=1 in the environment (read at every call) runs the same stepper on the host, a window a ycge_scene_hit batch. */
#define YCGE_CAMERA_MOVE_HORIZONTAL 0
#define YCGE_CAMERA_MOVE_VERTICAL 1
#define YCGE_CAMERA_MOVE_JUMP 2
#define YCGE_CAMERA_MOVE_SHIFT 3
#define YCGE_CAMERA_MAX_MOVES 32
#define YCGE_CAMERA_MAX_MOVE_LENGTH 64.0f
#define YCGE_CAMERA_MAX_MICRO_STEPS 1024
typedef struct ycge_camera_body {    /* 40 bytes */
    float pos[3];
    float vertical_velocity, shift_hold_timer;
    float repel_vel[3];
    int32_t auto_placed, is_grounded;
} ycge_camera_body;
typedef struct ycge_camera_world {   /* 12 bytes */
    float world_height, water_level, voxel_size_y;
} ycge_camera_world;
typedef struct ycge_camera_move {    /* 16 bytes */
    int32_t kind;                    /* YCGE_CAMERA_MOVE_* */
    int32_t shift;                   /* JUMP: the key came with Shift held */
    float a, b;                      /* HORIZONTAL: dx, dz; VERTICAL: dy */
} ycge_camera_move;
typedef struct ycge_camera_tick_info {   /* 12 uint32, 48 bytes */
    uint32_t rays_committed, rays_walked, windows;
    uint32_t micro_steps, blocked_steps, slides, push_outs, embedded_resolutions, ground_snaps, auto_placements, fail_safes;
    uint32_t reserved;
} ycge_camera_tick_info;
int ycge_volume_camera_tick(ycge_ctx *ctx, ycge_camera_body *body /* in, out */, const ycge_camera_world *world, const ycge_camera_move *moves,
                            int32_t n_moves, float delta_time_ms, int32_t run_update, ycge_camera_tick_info *info /* or NULL */);

/* --- many bodies of the voxel world a tick in one launch, each with its own shape (kernel k_bodies_tick in csrc/ycge_camera.hip, the
 * same stepper).  Added after ABI 10 without changing it: YCGE_ABI_VERSION stays 10, no existing struct changes; a host detects the
 * export by symbol lookup.
 * ycge_volume_camera_tick moves one body of one size: a host that also moves mobs, dropped items, projectiles or the other players of a
 * replicated scene pays one call, one launch, one read-back and one synchronise per body.  Here n independent bodies are one staged copy
 * up, one launch of n one-wavefront workgroups, one copy back and one synchronise, and every body comes back as the serial stepper leaves
 * it alone, bit for bit: body i's outcome is a function of its own inputs and the scene only - bodies do not see each other, the
 * position in the batch and the other bodies do not matter.
 *   bodies      n bodies (in, out), as ycge_volume_camera_tick's one.
 *   shapes      n shapes, or NULL: every body has YCGE_BODY_SHAPE_DEFAULT.  A shape is the reference's `const float` values that say how
 *               big a body is and how it jumps and falls (Scenes/VolumeScenes.cs:20-39): EyeHeight, CollisionRadius, ProbeRadius,
 *               GroundClearance, JumpSpeed, GravityAccel, read in the reference's types and order of operations.  MaxProbeHeight,
 *               LocalProbeDepthMin, LocalProbeStart, ExtraFallMargin, StepUpGuardEpsilon and ShiftHoldGraceSeconds stay the library's.
 *   moves,      body i applies moves[move_first[i] .. move_first[i + 1]) in order (at most YCGE_CAMERA_MAX_MOVES), then, when
 *   move_first  run_update != 0, Update's physics with delta_time_ms, exactly as ycge_volume_camera_tick does for one body.  move_first
 *               has n + 1 entries, starts at 0 and does not decrease.
 *   results     n records, all filled by a call that ran (it returns YCGE_OK): status 0 - bodies[i] and info[i] are the tick's; status
 *               1 (a horizontal move reached YCGE_CAMERA_MAX_MICRO_STEPS), 2 (a vertical move did), 3 (the position stopped being
 *               finite) - bodies[i] and info[i] are left as they were and bad_move is the body's own move index, or -1.  The other bodies
 *               commit all the same: one body in a corner does not cost the rest their tick.
 *   info        (may be NULL) n records of ycge_camera_tick_info.
 * The scene and the stream are ycge_volume_camera_tick's: the query stream, waits for the device work of the last scene change and NOT for
 * frames in flight, changes nothing a frame reads.  YCGE_ERR_NO_SCENE before the first upload; n = 0 with a scene: YCGE_OK.
 * Refused on the host before any device work with YCGE_ERR_INVALID_ARG, nothing written (results included), the message naming the body
 * and, where there is one, the move ("body 7: move 2: longer than ..."): a peer context; n outside 0..YCGE_BODIES_MAX; NULL bodies,
 * world, results or move_first with n > 0; NULL moves while some body has moves; move_first[0] != 0, a decreasing move_first, more than
 * YCGE_CAMERA_MAX_MOVES moves for one body; whatever ycge_volume_camera_tick refuses for a body, its moves, the world and the time step;
 * a shape with a field that is not finite, with eye_height, collision_radius, probe_radius or gravity_accel not positive, with
 * ground_clearance or jump_speed negative, or with eye_height or collision_radius above YCGE_BODY_SHAPE_MAX_SIZE (the caps on moves and
 * micro-steps keep their meaning).  A device error fails the call and writes nothing.
 * YCGE_CAMERA_HOST=1 in the environment (read at every call) runs the same stepper on the host: a round collects the next window of every
 * body still running into one ycge_scene_hit batch and commits body by body. */
#define YCGE_BODIES_MAX 4096
#define YCGE_BODY_SHAPE_MAX_SIZE 64.0f
typedef struct ycge_body_shape {     /* 24 bytes */
    float eye_height, collision_radius, probe_radius, ground_clearance, jump_speed, gravity_accel;
} ycge_body_shape;
#define YCGE_BODY_SHAPE_DEFAULT {1.7f, 0.65f, 0.35f, 0.10f, 4.8f, 9.81f}
typedef struct ycge_body_result {    /* 8 bytes */
    int32_t status;                  /* 0 committed; 1 a horizontal move reached YCGE_CAMERA_MAX_MICRO_STEPS; 2 a vertical move did; 3 the position stopped being finite */
    int32_t bad_move;                /* status 1..3: the body's own move index, or -1 */
} ycge_body_result;
int ycge_volume_bodies_tick(ycge_ctx *ctx, ycge_camera_body *bodies /* n, in, out */, const ycge_body_shape *shapes /* n, or NULL: the reference's */,
                            int32_t n, const ycge_camera_world *world, const ycge_camera_move *moves, const int32_t *move_first /* n + 1 */,
                            float delta_time_ms, int32_t run_update, ycge_body_result *results /* n */, ycge_camera_tick_info *info /* n, or NULL */);

/* tests only */
int ycge_read_buffer(ycge_ctx *ctx, int32_t which /* ycge_buffer */, void *dst, size_t bytes);
int ycge_set_frame_counter(ycge_ctx *ctx, int64_t frame_counter);
/* measurement: what the TIMED kernel instances (config.count_work == 0) have done since the context was created, all devices:
 * traversal-loop steps summed over lanes - one step = one node visit (a 64-byte record), one leaf record (72 bytes: two triangles)
 * or one voxel cell.  The counting instances walk the reference's full traversal (SURVEY 8d counters in ycge_frame_stats); the
 * timed ones stop shadow queries at the first hit and skip culled grids, so their own work is reported apart.  Waits for the
 * context's stream; never called inside a timed region. */
int ycge_read_timed_steps(ycge_ctx *ctx, uint64_t *lane_steps);
/* The SDR frame leaves the device by one copy into the caller's buffer at the end of ycge_render_frame / ycge_resolve_gathered (24 bytes per
 * chexel: 25 MB at 1920x540).  Into page-locked memory that copy is a DMA at the link's full rate instead of a staged copy into pageable
 * pages, and a frame in flight (ycge_render_frame_async_sdr) never blocks the calling thread.  Two ways to get such memory:
 *   ycge_alloc_host_buffer / ycge_free_host_buffer   the library's own (hipHostMalloc, zeroed): what a host should use for its SDR frames
 *                                                     (the C# wrapper reads it through a Span<float>);
 *   ycge_pin_host_buffer / ycge_unpin_host_buffer     registers memory the caller owns (hipHostRegister).  Registration is page-granular:
 *                                                     two registered ranges that share a page lose it when one is unregistered, and the
 *                                                     other's next read-back faults on the device.  So the range must be WHOLE PAGES OF ITS
 *                                                     OWN: `buffer` aligned to ycge_host_page_size() and `bytes` a multiple of it, else
 *                                                     YCGE_ERR_INVALID_ARG (a pinned managed array - GCHandle of a float[] - never qualifies).
 * ABI 8.  Optional either way; unpin / free before the memory goes away, and only after ycge_wait. */
size_t ycge_host_page_size(void);
int ycge_alloc_host_buffer(size_t bytes, void **out_buffer);
int ycge_free_host_buffer(void *buffer);
int ycge_pin_host_buffer(void *buffer, size_t bytes);
int ycge_unpin_host_buffer(void *buffer);
/* visible HIP devices (hipGetDeviceCount; does not initialise a device context), < 0 on error: what a host checks before it
 * fills config.devices[] */
int ycge_device_count(void);
int ycge_accel_size(ycge_ctx *ctx, int32_t which /* ycge_accel */, int32_t index, size_t *bytes);
int ycge_read_accel(ycge_ctx *ctx, int32_t which, int32_t index, void *dst, size_t bytes);
/* name of the device the context runs on + whether the gfx950 code object loaded */
int ycge_device_info(ycge_ctx *ctx, char *name, size_t name_bytes, int32_t *compute_units);

#ifdef __cplusplus
}
#endif
#endif /* YCGE_H */
