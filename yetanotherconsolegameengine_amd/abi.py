"""ctypes mirror of include/ycge.h — the C-ABI of the MI355X ray-trace core.

Every structure here has the same field order and types as its C twin; the
`-m "not gpu"` tests check sizes/offsets against the header through the built
library (ycge_abi_sizeof).  The product library is libycge_hip.so (host C++ +
gfx950 HIP kernels); there is NO CPU fallback: if the library or its device
code is missing, loading or ycge_create fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

YCGE_ABI_VERSION = 10
YCGE_MAX_DEVICES = 8

# ycge_status
YCGE_OK = 0
YCGE_ERR_INVALID_ARG = -1
YCGE_ERR_NO_SCENE = -2
YCGE_ERR_DEVICE = -3
YCGE_ERR_UNSUPPORTED = -4
YCGE_ERR_OUT_OF_MEMORY = -5
YCGE_ERR_STACK_DEPTH = -6
YCGE_ERR_NO_DEVICE_CODE = -7
YCGE_ERR_INTERNAL = -8

STATUS_NAMES = {
    0: "YCGE_OK", -1: "YCGE_ERR_INVALID_ARG", -2: "YCGE_ERR_NO_SCENE", -3: "YCGE_ERR_DEVICE",
    -4: "YCGE_ERR_UNSUPPORTED", -5: "YCGE_ERR_OUT_OF_MEMORY", -6: "YCGE_ERR_STACK_DEPTH",
    -7: "YCGE_ERR_NO_DEVICE_CODE",
    -8: "YCGE_ERR_INTERNAL",
}

# ycge_exchange
EXCHANGE_PEER_PUSH, EXCHANGE_RCCL = 0, 1
# ycge_material_kind
MAT_CONSTANT, MAT_CHECKER, MAT_TEXTURED = 0, 1, 2
# ycge_prim_type
(PRIM_SPHERE, PRIM_PLANE, PRIM_DISK, PRIM_XYRECT, PRIM_XZRECT, PRIM_YZRECT, PRIM_BOX,
 PRIM_CYLINDER_Y, PRIM_TRIANGLE, PRIM_MESH, PRIM_VOLUME_GRID) = range(11)
# ycge_buffer
(BUF_RAYS, BUF_PRIM_ID, BUF_SUB_ID, BUF_HIT_T, BUF_CURRENT_HDR, BUF_G_ALBEDO, BUF_G_NORMAL,
 BUF_G_DEPTH, BUF_SKY_MASK, BUF_TAA_HISTORY, BUF_PREV_NORMAL, BUF_PREV_DEPTH, BUF_PREV_SKY,
 BUF_DENOISED, BUF_RNG_STATE) = range(15)
# ycge_accel
ACCEL_SCENE_NODES, ACCEL_SCENE_LEAF_INDEX, ACCEL_MESH_NODES, ACCEL_MESH_LEAF_INDEX = range(4)

# (numpy dtype, elements per pixel) of each per-pixel buffer
BUFFER_LAYOUT = {
    BUF_RAYS: ("<f4", 6), BUF_PRIM_ID: ("<i4", 1), BUF_SUB_ID: ("<i4", 1), BUF_HIT_T: ("<f4", 1),
    BUF_CURRENT_HDR: ("<f4", 3), BUF_G_ALBEDO: ("<f4", 3), BUF_G_NORMAL: ("<f4", 3), BUF_G_DEPTH: ("<f4", 1),
    BUF_SKY_MASK: ("u1", 1), BUF_TAA_HISTORY: ("<f4", 3), BUF_PREV_NORMAL: ("<f4", 3),
    BUF_PREV_DEPTH: ("<f4", 1), BUF_PREV_SKY: ("u1", 1), BUF_DENOISED: ("<f4", 3), BUF_RNG_STATE: ("<u8", 1),
}


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Material(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("albedo", Vec3), ("albedo_b", Vec3), ("checker_scale", C.c_float),
        ("specular", C.c_float), ("reflectivity", C.c_float), ("emission", Vec3),
        ("transparency", C.c_float), ("index_of_refraction", C.c_float), ("transmission_color", Vec3),
        ("texture", C.c_int32), ("reserved", C.c_int32), ("texture_weight", C.c_double), ("uv_scale", C.c_double),
    ]


class Texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pixels", C.POINTER(C.c_uint32)),
                ("frame_bytes_per_pixel", C.c_int32), ("flip_u", C.c_int32), ("flip_v", C.c_int32), ("frame", C.POINTER(C.c_uint8))]


class Prim(C.Structure):
    _fields_ = [
        ("type", C.c_int32), ("material", C.c_int32), ("ref", C.c_int32), ("reserved", C.c_int32),
        ("p", C.c_float * 12), ("specular", C.c_float), ("reflectivity", C.c_float),
    ]


class Mesh(C.Structure):
    _fields_ = [
        ("triangles", C.POINTER(C.c_float)), ("n_triangles", C.c_int32), ("material", C.c_int32),
        ("tri_material", C.POINTER(C.c_int32)),
    ]


class VoxelLookup(C.Structure):
    _fields_ = [("mat_id", C.c_int32), ("meta_id", C.c_int32), ("material", C.c_int32)]


class Grid(C.Structure):
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("min_corner", Vec3), ("voxel_size", Vec3),
        ("cells", C.POINTER(C.c_int32)), ("lookup", C.POINTER(VoxelLookup)), ("n_lookup", C.c_int32),
        ("default_material", C.c_int32), ("wireframe", C.c_int32), ("wire_width_fraction", C.c_float),
        ("wire_max_distance", C.c_float),
    ]


class VoxelEdit(C.Structure):
    """ycge_voxel_edit (36 bytes): every cell of the inclusive index box lo..hi of a resident grid - or, for ycge_world_store_edit, of the
    store, with grid_index 0 - becomes (mat_id, meta_id)."""
    _fields_ = [("grid_index", C.c_int32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("mat_id", C.c_int32), ("meta_id", C.c_int32)]


VOXEL_EDIT_MAX_OPS = 1 << 20
VOXEL_EDIT_INFO = ("cells_changed", "bricks_written", "records_changed", "objects_installed")


class CameraBody(C.Structure):
    """ycge_camera_body (40 bytes): what VolumeScene keeps between ticks - CameraPos, verticalVelocity, shiftHoldTimer, repelVel, autoPlaced,
    isGrounded (ycge_volume_camera_tick)."""
    _fields_ = [("pos", C.c_float * 3), ("vertical_velocity", C.c_float), ("shift_hold_timer", C.c_float), ("repel_vel", C.c_float * 3),
                ("auto_placed", C.c_int32), ("is_grounded", C.c_int32)]


class CameraWorld(C.Structure):
    """ycge_camera_world (12 bytes): WorldConfig's WorldHeight, WaterLevel and VoxelSize.Y."""
    _fields_ = [("world_height", C.c_float), ("water_level", C.c_float), ("voxel_size_y", C.c_float)]


class CameraMove(C.Structure):
    """ycge_camera_move (16 bytes): one HandleInput call's effect on the body.  HORIZONTAL: a, b = dx, dz; VERTICAL: a = dy; JUMP: shift = the key
    came with Shift held; SHIFT: the fly timer is refreshed."""
    _fields_ = [("kind", C.c_int32), ("shift", C.c_int32), ("a", C.c_float), ("b", C.c_float)]


class CameraTickInfo(C.Structure):
    """ycge_camera_tick_info (12 uint32)"""
    _fields_ = [(n, C.c_uint32) for n in ("rays_committed", "rays_walked", "windows", "micro_steps", "blocked_steps", "slides", "push_outs",
                                          "embedded_resolutions", "ground_snaps", "auto_placements", "fail_safes", "reserved")]


CAMERA_MOVE_HORIZONTAL, CAMERA_MOVE_VERTICAL, CAMERA_MOVE_JUMP, CAMERA_MOVE_SHIFT = 0, 1, 2, 3
CAMERA_MAX_MOVES = 32
CAMERA_MAX_MOVE_LENGTH = 64.0
CAMERA_MAX_MICRO_STEPS = 1024


class BodyShape(C.Structure):
    """ycge_body_shape (24 bytes): how big a body is and how it jumps and falls - the reference's EyeHeight, CollisionRadius, ProbeRadius,
    GroundClearance, JumpSpeed, GravityAccel (Scenes/VolumeScenes.cs:20-39) as data (ycge_volume_bodies_tick)."""
    _fields_ = [(n, C.c_float) for n in ("eye_height", "collision_radius", "probe_radius", "ground_clearance", "jump_speed", "gravity_accel")]


class BodyResult(C.Structure):
    """ycge_body_result (8 bytes): status 0 committed, 1 / 2 a horizontal / vertical move reached CAMERA_MAX_MICRO_STEPS, 3 the position stopped
    being finite; bad_move the body's own move index, or -1."""
    _fields_ = [("status", C.c_int32), ("bad_move", C.c_int32)]


BODIES_MAX = 4096
BODY_SHAPE_MAX_SIZE = 64.0
BODY_SHAPE_DEFAULT = (1.7, 0.65, 0.35, 0.10, 4.8, 9.81)          # YCGE_BODY_SHAPE_DEFAULT: the reference's
# int hit(void *user, const float ray[8], float rec[7]) of ycge_test_camera_tick_host (include/ycge_hooks.h)
CAMERA_HIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float))


class World(C.Structure):
    """ycge_world: WorldConfig as a chunk depends on it (ycge_worldgen_chunk_cells / ycge_scene_generate_grids)."""
    _fields_ = [("chunk_size", C.c_int32), ("chunks_y", C.c_int32), ("world_seed", C.c_int32), ("world_min", Vec3), ("voxel_size", Vec3)]


class Light(C.Structure):
    _fields_ = [("position", Vec3), ("color", Vec3), ("intensity", C.c_float)]


class Scene(C.Structure):
    _fields_ = [
        ("materials", C.POINTER(Material)), ("n_materials", C.c_int32),
        ("prims", C.POINTER(Prim)), ("n_prims", C.c_int32),
        ("meshes", C.POINTER(Mesh)), ("n_meshes", C.c_int32),
        ("grids", C.POINTER(Grid)), ("n_grids", C.c_int32),
        ("lights", C.POINTER(Light)), ("n_lights", C.c_int32),
        ("ambient_color", Vec3), ("ambient_intensity", C.c_float),
        ("background_top", Vec3), ("background_bottom", Vec3),
        ("is_volume_scene", C.c_int32), ("n_textures", C.c_int32), ("textures", C.POINTER(Texture)),
        ("has_dynamic_textures", C.c_int32),
    ]


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("fb_width", C.c_int32), ("fb_height", C.c_int32), ("super_sample", C.c_int32),
        ("fov_deg", C.c_float), ("device", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32),
        ("diffuse_bounces", C.c_int32), ("max_mirror_bounces", C.c_int32), ("max_refractions", C.c_int32),
        ("mirror_threshold", C.c_float), ("eps", C.c_float), ("seed_salt", C.c_uint64),
        ("taa_alpha", C.c_float), ("motion_trans_reset", C.c_float), ("motion_rot_reset", C.c_float),
        ("diffuse_sigma_deg", C.c_float), ("taa_clamp_radius", C.c_int32), ("taa_luminance_pad", C.c_float),
        ("atrous_iterations", C.c_int32), ("atrous_c_phi", C.c_float), ("atrous_n_phi", C.c_float),
        ("atrous_z_phi", C.c_float), ("atrous_a_phi", C.c_float), ("capture_debug", C.c_int32),
        ("count_work", C.c_int32),
        ("slab_albedo", C.c_int32),
        ("n_devices", C.c_int32), ("devices", C.c_int32 * YCGE_MAX_DEVICES),
        ("atrous_inplace_exact", C.c_int32), ("tile_ring", C.c_int32), ("multi_device_exchange", C.c_int32),
    ]


class FrameStats(C.Structure):
    _fields_ = [
        ("frame", C.c_int64), ("history_reset", C.c_int32), ("fan_blocks", C.c_int32),      # fan_blocks: reserved, always 0
        ("trace_ms", C.c_double), ("taa_ms", C.c_double), ("post_ms", C.c_double), ("total_ms", C.c_double),
        ("n_rays", C.c_uint64), ("n_box", C.c_uint64), ("n_tri", C.c_uint64), ("n_prim", C.c_uint64),
        ("n_vox", C.c_uint64), ("exposure", C.c_float), ("exposure_serial_chunks", C.c_float),
        ("n_rays_dark", C.c_uint64), ("n_devices_traced", C.c_int32), ("device_tiles", C.c_int32 * 8),
    ]


class ObjInfo(C.Structure):
    """ycge_obj_info: what ycge_obj_parse / ycge_obj_parse_host found (passed with C.byref)."""
    _fields_ = [("n_positions", C.c_int32), ("n_triangles", C.c_int32), ("n_lines", C.c_int64), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class ObjGroundInfo(C.Structure):
    """ycge_obj_ground_info, 64 bytes: what ycge_obj_ground / ycge_obj_ground_host found (passed with C.byref)."""
    _fields_ = [("min", C.c_float * 3), ("max", C.c_float * 3), ("centroid", C.c_float * 3), ("extent", C.c_float), ("n_components", C.c_int32),
                ("component_faces", C.c_int32), ("component_vertices", C.c_int32), ("first_face", C.c_int32), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class Chexel(C.Structure):
    """ycge_chexel, 28 bytes: Chexel.Char as its UTF-16 code unit, ForegroundColor.color_f32, BackgroundColor.color_f32."""
    _fields_ = [("ch", C.c_uint16), ("pad", C.c_uint16), ("fg", C.c_float * 3), ("bg", C.c_float * 3)]


class ConsoleLayer(C.Structure):
    """ycge_console_layer: a Framebuffer's ViewportX, ViewportY, Width, Height and its cells row by row (cell (x, y) at y * w + x)."""
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("cells", C.POINTER(Chexel))]


CONSOLE_MAX_LAYERS = 16


class FlightInfo(C.Structure):
    _fields_ = [("two_trace_streams", C.c_int32), ("placed_gate", C.c_int32), ("post_gate", C.c_int32), ("post_pair", C.c_int32),
                ("frames_outstanding", C.c_int32), ("stage_pipeline", C.c_int32), ("placed_waits", C.c_uint64)]


class AnsiAsync(C.Structure):
    """ycge_ansi_async: the request of ycge_render_frame_async_ansi (ycge_abi_sizeof(12))."""
    _fields_ = [("console_w", C.c_int32), ("console_h", C.c_int32), ("viewport_x", C.c_int32), ("viewport_y", C.c_int32),
                ("default_fg16", C.c_int32), ("default_bg16", C.c_int32), ("clear_screen", C.c_int32), ("rgb", C.c_int32), ("delta", C.c_int32),
                ("merge_gap", C.c_int32), ("tolerance", C.c_int32), ("keyframe", C.c_int32)]


class AnsiAsyncResult(C.Structure):
    """ycge_ansi_async_result: the record k_ansi_deliver fills, in page-locked memory (ycge_abi_sizeof(13))."""
    _fields_ = [("length", C.c_uint64), ("info", C.c_uint32 * 4), ("status", C.c_uint32), ("reserved", C.c_uint32)]


ABI_SIZEOF_ANSI_ASYNC, ABI_SIZEOF_ANSI_ASYNC_RESULT = 12, 13


def default_config() -> Config:
    """Reference defaults (RaytraceRenderer.cs:31-43,65,218-224) — pure data, no library needed."""
    c = Config()
    c.abi_version = YCGE_ABI_VERSION
    c.fb_width, c.fb_height, c.super_sample = 80, 45, 1
    c.fov_deg = 45.0
    c.device, c.rank, c.world_size = 0, 0, 1
    c.diffuse_bounces, c.max_mirror_bounces, c.max_refractions = 1, 2, 2
    c.mirror_threshold, c.eps = 0.9, 1e-4
    c.seed_salt = 0x9E3779B97F4A7C15
    c.taa_alpha, c.motion_trans_reset, c.motion_rot_reset = 0.01, 0.0025, 0.0025
    c.diffuse_sigma_deg = 25.0
    c.taa_clamp_radius, c.taa_luminance_pad = 1, 0.10
    c.atrous_iterations = 3
    c.atrous_c_phi, c.atrous_n_phi, c.atrous_z_phi, c.atrous_a_phi = 3.0, 0.35, 2.0, 0.20
    c.capture_debug, c.count_work = 0, 0
    c.slab_albedo, c.n_devices = 1, 0
    c.atrous_inplace_exact = 1
    c.tile_ring = 0
    c.multi_device_exchange = EXCHANGE_PEER_PUSH
    return c


_PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = _PKG_DIR / "lib" / "libycge_hip.so"

# name -> (restype, argtypes); every symbol include/ycge.h declares
_PROTOTYPES = {
    "ycge_config_default": (C.c_int, [C.POINTER(Config)]),
    "ycge_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "ycge_destroy": (None, [C.c_void_p]),
    "ycge_last_error": (C.c_char_p, [C.c_void_p]),
    "ycge_scene_upload": (C.c_int, [C.c_void_p, C.POINTER(Scene)]),
    "ycge_validate_scene": (C.c_int, [C.POINTER(Scene), C.c_char_p, C.c_size_t]),
    "ycge_scene_update_lights": (C.c_int, [C.c_void_p, C.POINTER(Light), C.c_int32, C.POINTER(Vec3), C.c_float,
                                           C.POINTER(Vec3), C.POINTER(Vec3)]),
    "ycge_scene_update_objects": (C.c_int, [C.c_void_p, C.POINTER(Prim), C.c_int32]),
    "ycge_scene_attach_grids": (C.c_int, [C.c_void_p, C.POINTER(Grid), C.c_int32, C.POINTER(C.c_int32)]),
    "ycge_scene_detach_grids": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "ycge_scene_attach_meshes": (C.c_int, [C.c_void_p, C.POINTER(Mesh), C.c_int32, C.POINTER(C.c_int32)]),
    "ycge_scene_detach_meshes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "ycge_scene_append_materials": (C.c_int, [C.c_void_p, C.POINTER(Material), C.c_int32, C.POINTER(C.c_int32)]),
    # (translate_or_target: 3 floats or None; out_bounds: 6 floats or None)
    "ycge_scene_attach_obj_mesh": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32), C.c_void_p]),
    # (world: a ycge_world, passed with C.byref(abi.World))
    "ycge_worldgen_chunk_cells": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ycge_scene_generate_grids": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(Grid), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ycge_worldgen_world_cells": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "ycge_scene_generate_world": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Grid), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    # the world store: a VG01 payload resident on the device, chunks attached by key (keys: int32 [n, 3]; occupied_out: uint8 per chunk or None)
    "ycge_world_file_info": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]),
    "ycge_world_store_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ycge_world_store_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_size_t]),
    "ycge_scene_attach_world_chunks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(Grid), C.POINTER(C.c_int32)]),
    "ycge_world_store_release": (C.c_int, [C.c_void_p]),
    # the store made by the generator on the device (world: C.byref(abi.World); form: WORLD_STORE_FIELDS / WORLD_STORE_CELLS) and its x-planes read back (cells_out: int32 [planes, ny, nz, 2])
    "ycge_world_store_generate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "ycge_world_store_read": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    # voxel edits of resident grids and of the world store (ops: an array of abi.VoxelEdit; out_info: uint32 [4] or None)
    "ycge_scene_edit_voxels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)]),
    "ycge_world_store_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    # the pool of materialised chunks that lets a fields store take edits (keys: int32 [n, 3])
    "ycge_world_store_reserve_edits": (C.c_int, [C.c_void_p, C.c_int32]),
    "ycge_world_store_edit_slots": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ycge_world_store_revert_chunks": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]),
    "ycge_scene_update_texture": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "ycge_resize": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "ycge_set_camera": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_float]),
    "ycge_render_frame": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_render_frame_async": (C.c_int, [C.c_void_p]),
    "ycge_render_frame_async_sdr": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ycge_wait": (C.c_int, [C.c_void_p]),
    "ycge_async_trace_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_int32)]),
    "ycge_flight_query": (C.c_int, [C.c_void_p, C.POINTER(FlightInfo)]),
    "ycge_exchange_query": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ycge_tile_slab_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "ycge_trace_tiles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FrameStats)]),
    "ycge_resolve_gathered": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_halo_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ycge_history_slab_bytes": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "ycge_trace_tiles_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FrameStats)]),
    "ycge_trace_tiles_resident_batch": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_void_p), C.c_void_p]),
    "ycge_resolve_tiles_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FrameStats)]),
    "ycge_unpack_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_scene_hit": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "ycge_scene_occluded": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(C.c_uint8)]),
    # the camera tick (body / world / moves / info: CameraBody, CameraWorld, CameraMove[n], CameraTickInfo by address)
    "ycge_volume_camera_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p]),
    # many bodies a tick (bodies / shapes / n / world / moves / move_first / dt / run_update / results / info: CameraBody[n], BodyShape[n] or None,
    # CameraWorld, CameraMove[], int32[n + 1], BodyResult[n], CameraTickInfo[n] or None, by address)
    "ycge_volume_bodies_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p,
                                          C.c_void_p]),
    "ycge_render_frame_chexels": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                            C.POINTER(FrameStats)]),
    "ycge_render_frame_async_chexels": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "ycge_ansi_stream_bound": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "ycge_render_frame_ansi": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                         C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_video_blit": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                  C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]),
    "ycge_video_blit_ansi": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    # (out_info: 4 uint32 {keyframe returned, changed cells, emitted cells, run starts}, or None)
    "ycge_render_frame_ansi_delta": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                               C.POINTER(FrameStats)]),
    "ycge_video_blit_ansi_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t),
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    # the 24-bit colour forms of the five above (the _delta ones take `tolerance` behind merge_gap)
    "ycge_ansi_rgb_stream_bound": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "ycge_render_frame_ansi_rgb": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                             C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_render_frame_ansi_rgb_delta": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                   C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                                   C.POINTER(FrameStats)]),
    "ycge_video_blit_ansi_rgb": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    "ycge_video_blit_ansi_rgb_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t,
                                                 C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    # (layers: an array of abi.ConsoleLayer, or None with n = 0)
    "ycge_console_set_layers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    # the quadrant-glyph frames: the planes (SDR, 12 f32 a chexel, code units, fitted RGBA; min_contrast), the full stream (min_contrast behind
    # clear_screen) and the delta (min_contrast behind keyframe)
    "ycge_render_frame_quadrants": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.c_int32,
                                              C.POINTER(FrameStats)]),
    "ycge_render_frame_ansi_quad": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_render_frame_ansi_quad_delta": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                                    C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    # ... and of a video frame: the video calls' arguments with min_contrast where the frame forms have it
    "ycge_video_blit_quadrants": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                            C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.c_int32]),
    "ycge_video_blit_ansi_quad": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    "ycge_video_blit_ansi_quad_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t,
                                                  C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    # the sixel frames: the bound of a W x H picture; the planes (SDR, W x H RGBA8, W x H registers; dither); the stream (viewport, clear, dither);
    # the host encoder of a register plane (no context)
    "ycge_sixel_stream_bound": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "ycge_render_frame_pixels": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(FrameStats)]),
    "ycge_render_frame_sixel": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_sixel_encode_host": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
    # sixel in Video mode (the planes; the stream) and the delta sixel streams of frames and video (keyframe; out_info: 4 words or None), and the host
    # encoder of the delta between two register planes (no context)
    "ycge_video_blit_pixels": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                         C.POINTER(C.c_uint8), C.c_int32]),
    "ycge_video_blit_sixel": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_float)]),
    "ycge_render_frame_sixel_delta": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t,
                                                C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_video_blit_sixel_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "ycge_sixel_encode_delta_host": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t,
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
    # the adaptive sixel palette: the bound; the stream of a frame / a video source (viewport, clear, hold; palette 256 x RGBA8 and count, either None);
    # the planes (SDR, RGBA, registers, hold, palette, count); the rule and the stream in plain C++ (no context)
    "ycge_sixel_palette_stream_bound": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "ycge_render_frame_sixel_palette": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(FrameStats)]),
    "ycge_video_blit_sixel_palette": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
    "ycge_render_frame_pixels_palette": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_uint8),
                                                   C.POINTER(C.c_int32), C.POINTER(FrameStats)]),
    "ycge_video_blit_pixels_palette": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_uint8),
                                                 C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "ycge_sixel_palette_host": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]),
    "ycge_sixel_encode_palette_host": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    # (req: C.byref(abi.AnsiAsync); out_result: the address of an abi.AnsiAsyncResult in page-locked memory)
    "ycge_render_frame_async_ansi": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]),
    # (info: a ycge_obj_info, passed with C.byref(abi.ObjInfo))
    "ycge_obj_parse_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]),
    "ycge_obj_parse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ycge_obj_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_obj_triangles": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    "ycge_obj_release": (C.c_int, [C.c_void_p]),
    # (out / out_info: a ycge_obj_ground_info, passed with C.byref(abi.ObjGroundInfo); out_info may be None)
    "ycge_obj_ground_host": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "ycge_obj_ground": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ycge_obj_triangles_auto_ground": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_read_buffer": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]),
    "ycge_set_frame_counter": (C.c_int, [C.c_void_p, C.c_int64]),
    "ycge_read_timed_steps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "ycge_device_count": (C.c_int, []),
    "ycge_host_page_size": (C.c_size_t, []),
    "ycge_alloc_host_buffer": (C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    "ycge_free_host_buffer": (C.c_int, [C.c_void_p]),
    "ycge_pin_host_buffer": (C.c_int, [C.c_void_p, C.c_size_t]),
    "ycge_unpin_host_buffer": (C.c_int, [C.c_void_p]),
    "ycge_accel_size": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "ycge_read_accel": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]),
    "ycge_device_info": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32)]),
}
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

# test / profiling hooks of chunk streaming (include/ycge_hooks.h; not part of the boundary)
GGRID_BYTES = 112
HOOK_PROTOTYPES = {
    "ycge_debug_read_grid": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "ycge_debug_grid_pool_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ycge_debug_peer_context": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "ycge_debug_live_resources": (C.c_int, [C.POINTER(C.c_int64)]),
}
# the camera physics' stepper on the host over a caller's Scene.Hit (csrc/ycge_camera.cpp), bound where it is used (VolumeCamera.tick_host)
CAMERA_HOOK_PROTOTYPES = {
    "ycge_test_camera_tick_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, CAMERA_HIT_FN, C.c_void_p,
                                             C.c_int32, C.c_char_p, C.c_size_t]),
    "ycge_test_bodies_tick_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                             CAMERA_HIT_FN, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]),
}
# test / profiling hook of chunk generation (csrc/ycge_worldgen_scene.cpp), bound where it is used (RaytraceRenderer.worldgen_stats)
WORLDGEN_HOOK_PROTOTYPES = {
    "ycge_debug_worldgen_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ycge_debug_worldpregen_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ycge_host_worldgen_world_fields": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 10),
    "ycge_host_worldgen_river_global": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "ycge_host_worldgen_world_from_fields": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
}
# test / profiling hooks of the world store (csrc/ycge_world_store.cpp), bound where they are used (RaytraceRenderer.world_store_chunk / world_store_stats)
WORLD_STORE_HOOK_PROTOTYPES = {
    "ycge_debug_world_store_chunk": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "ycge_debug_world_store_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ycge_debug_world_store_generate_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
}
WORLD_STORE_FIELDS, WORLD_STORE_CELLS = 0, 1          # ycge_world_store_generate's form (YCGE_WORLD_STORE_FIELDS / _CELLS)
WORLD_STORE_FORMS = {"fields": WORLD_STORE_FIELDS, "cells": WORLD_STORE_CELLS}
WORLD_STORE_GENERATE_STATS = ("form", "on_host", "any_leaves_passes", "plane_slabs", "fields_us", "any_leaves_us", "occupied_us", "planes_us", "host_generator_us")
WORLD_STORE_STATS = ("store_bytes", "slabs", "load_stage_us", "load_h2d_us", "load_occupied_us", "last_slice_us", "device_chunks", "host_chunks")
# test hooks of the post stage on caller-given inputs (csrc/ycge_post_host.cpp), bound where they are used (RaytraceRenderer.post_probe /
# exposure_probe); state_out: POST_STATE_WORDS uint32
POST_HOOK_PROTOTYPES = {
    "ycge_test_post_stage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_test_exposure": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int32, C.c_void_p]),
}
POST_STATE_WORDS = 6
# test hook of TemporalBlendWithClamp on caller-given planes (csrc/ycge_resident.cpp), bound where it is used (RaytraceRenderer.taa_probe): form, reset,
# w, h, the eight input planes, taa_alpha, taa_clamp_radius, taa_luminance_pad, history / normal / depth / sky out, the history slab (tile forms) or None
TAA_HOOK_PROTOTYPES = {
    "ycge_test_taa": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 8 + [C.c_float, C.c_int32, C.c_float] + [C.c_void_p] * 5),
}
TAA_FORM_PLANES, TAA_FORM_IN_PLACE, TAA_FORM_KEEP_PLANES, TAA_FORM_IN_FLIGHT, TAA_FORM_SCATTER_TILES, TAA_FORM_RESOLVE_TILES = range(6)
# test hooks of Video mode (csrc/ycge_video.cpp), bound where they are used (renderer.video_tables / VideoRenderer.blit_probe)
VIDEO_HOOK_PROTOTYPES = {
    "ycge_host_video_tables": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_test_video_blit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "ycge_test_video_blit_quadrants": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
}
# test hook of the delta ANSI stream (csrc/ycge_ansi.cpp), bound where it is used (tests/test_gpu_ansi_delta.py)
ANSI_DELTA_HOOK_PROTOTYPES = {
    "ycge_test_ansi_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)] + [C.c_int32] * 10 +
                             [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
}
# test hooks of the 24-bit colour streams (csrc/ycge_ansi.cpp), bound where they are used (tests/test_gpu_ansi_rgb.py): the planes are
# fbW x 2 fbH RGBA8; the delta hook's last argument is out_shown (or None)
ANSI_RGB_HOOK_PROTOTYPES = {
    "ycge_test_ansi_rgb_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)] + [C.c_int32] * 9 + [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "ycge_test_ansi_rgb_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)] + [C.c_int32] * 11 +
                                 [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
}
# test hook of the layered streams (csrc/ycge_ansi.cpp), bound where it is used (tests/test_gpu_ansi_layers.py): rgb, the framebuffer plane,
# fbW, fbH, the layers (an array of abi.ConsoleLayer), n, raytrace_at, the previous composite's colours and glyphs (or None), the console,
# viewport, defaults and clear_screen, delta, merge_gap, tolerance, the stream's four arguments, the next composite's colours and glyphs (or None)
ANSI_LAYERS_HOOK_PROTOTYPES = {
    "ycge_test_ansi_layers": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                        C.POINTER(C.c_uint16)] + [C.c_int32] * 10 +
                              [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)]),
}
# test hooks of the quadrant-glyph frames (csrc/ycge_chexel.cpp, csrc/ycge_ansi.cpp), bound where they are used (tests/test_gpu_quadrants.py):
# the two kernels alone, and the streams on given glyph (uint16) + RGBA planes; the delta hook starts with the shown composite's colours and
# glyphs (or None) and ends with the next such (or None)
QUADRANT_HOOK_PROTOTYPES = {
    "ycge_test_quadrant_sdr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]),
    "ycge_test_quadrant_fit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "ycge_test_ansi_quad_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)] + [C.c_int32] * 9 +
                                   [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "ycge_test_ansi_quad_delta": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)] + [C.c_int32] * 11 +
                                  [C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)]),
}
# test hooks of the sixel frames (csrc/ycge_sixel.cpp), bound where they are used (tests/test_gpu_sixel.py): the pixel stage alone on a hi-res
# buffer (fbW, fbH, ss, exposure, dither; RGBA and register planes, either None), the encoder alone on a register plane (W, H, vx, vy, clear)
SIXEL_HOOK_PROTOTYPES = {
    "ycge_test_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    "ycge_test_sixel_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_size_t,
                                         C.POINTER(C.c_size_t)]),
}
# ... and of their Video mode and delta forms (tests/test_gpu_video_sixel.py, tests/test_gpu_sixel_delta.py; a table of its own: the one above
# is held to its two names by tests/test_sixel_cpu.py): k_video_pixels alone on a source frame and geometry (src_w, src_h, bpp, fbW, fbH, ss,
# dither; the planes, either None), the delta encoder alone on two register planes (prev, cur, W, H, vx, vy; out_info 4 words or None)
SIXEL_DELTA_HOOK_PROTOTYPES = {
    "ycge_test_video_pixels": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p]),
    "ycge_test_sixel_delta_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                               C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]),
}
# ... and of the adaptive palette (tests/test_gpu_sixel_palette.py): the palette stage alone on an RGBA plane (W, H, hold; registers, palette, percentages,
# count, any None), and the stage with the 256-register encoder (W, H, vx, vy, clear, hold)
SIXEL_PALETTE_HOOK_PROTOTYPES = {
    "ycge_test_sixel_palette": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                          C.POINTER(C.c_int32)]),
    "ycge_test_sixel_palette_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                                 C.c_size_t, C.POINTER(C.c_size_t)]),
}
# test hook of the delivery of a stream with frames in flight (csrc/ycge_ansi.cpp), bound where it is used (tests/test_gpu_ansi_flight.py): src,
# n_src, length, capacity, keyframe, counts (3 uint32), groups, out_stream, out_result (an abi.AnsiAsyncResult in page-locked memory)
ANSI_FLIGHT_HOOK_PROTOTYPES = {
    "ycge_test_ansi_deliver": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_size_t, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.c_void_p,
                                         C.c_void_p]),
}
# test / profiling hooks of the device-side mesh BVH build (csrc/ycge_mesh_bvh.cpp), bound where they are used (RaytraceRenderer.mesh_bvh_stats,
# device_mesh_bvh below); res16: MESH_BVH_RES_WORDS uint32, the fallback reasons as the library names them
MESH_BVH_HOOK_PROTOTYPES = {
    "ycge_debug_device_mesh_bvh": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_debug_mesh_bvh_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
}
MESH_BVH_RES_WORDS = 16
MESH_BVH_STATS = ("device_builds", "host_builds", "host_fallbacks", "last_device_build_us", "sort_fallbacks", "max_depth", "wide_nodes", "subtree_workgroups")
MESH_BVH_BUILT, MESH_BVH_SORT_NO_SPLIT, MESH_BVH_SORT_EMPTY_SIDE, MESH_BVH_TOP_OVERFLOW, MESH_BVH_TOO_DEEP, MESH_BVH_NON_FINITE = range(6)
# test / profiling hooks of the arena assembled on the device (csrc/ycge_mesh_emit.hip), bound where they are used (RaytraceRenderer.mesh_emit_stats /
# read_mesh_arena, device_mesh_arena in the tests); res8: MESH_EMIT_RES_WORDS uint32
MESH_EMIT_HOOK_PROTOTYPES = {
    "ycge_debug_device_mesh_arena": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ycge_debug_read_mesh_arena": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ycge_debug_read_meshes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "ycge_debug_mesh_emit_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
}
MESH_EMIT_RES_WORDS = 8
MESH_EMIT_RES = ("tree_built_on_device", "nodes", "record_units", "layout_us", "records_us", "treelets_us")
MESH_EMIT_STATS = ("device_meshes", "host_meshes", "last_device_emit_us", "arena_bytes")
# test / profiling hooks of the pool of resident meshes (csrc/ycge_mesh_pool.cpp), bound where they are used (RaytraceRenderer.mesh_pool_stats, mesh_ranges below)
MESH_POOL_HOOK_PROTOTYPES = {
    "ycge_debug_mesh_pool_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ycge_debug_mesh_ranges": (C.c_int, [C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
}
MESH_POOL_STATS = ("resident", "free_indices", "units_in_use", "capacity_units", "growths", "ranges_reused", "device_builds", "host_builds",
                   "build_us", "emit_us", "copy_us", "pooled")
MESH_RANGE_TAKE, MESH_RANGE_GIVE, MESH_INDEX_TAKE, MESH_INDEX_GIVE = range(4)

# test / profiling hook of the OBJ parse (csrc/ycge_obj.cpp), bound where it is used (RaytraceRenderer.obj_stats, obj_geometry below)
OBJ_HOOK_PROTOTYPES = {
    "ycge_debug_obj_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
}
OBJ_STATS = ("device_parses", "host_parses", "last_decline", "lines_us", "parse_us", "triangles_us")
OBJ_DECLINE_FLOAT_DOMAIN, OBJ_DECLINE_LINE_CAP, OBJ_DECLINE_ENV_HOST, OBJ_DECLINE_BELOW_MIN = 1, 2, 4, 8
# ... and of the auto-ground tail (csrc/ycge_obj_ground.hip), bound where they are used (RaytraceRenderer.obj_ground_stats, obj_ground_geometry below)
OBJ_GROUND_HOOK_PROTOTYPES = {
    "ycge_debug_obj_ground_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ycge_debug_obj_ground_phases": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
}
OBJ_GROUND_STATS = ("device_tails", "host_tails", "last_decline", "rounds", "serial_sums", "last_us")
OBJ_GROUND_PHASES = ("label_us", "select_us", "terms_us", "sums_us", "bounds_us")
OBJ_GROUND_DECLINE_FIND_BOUND, OBJ_GROUND_DECLINE_ROUND_CAP, OBJ_GROUND_DECLINE_ENV_HOST, OBJ_GROUND_DECLINE_BELOW_MIN = 1, 2, 4, 8

_lib = None


class YcgeError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


def bind(lib: C.CDLL, prefix: str = "ycge_", names=None) -> C.CDLL:
    """Attach prototypes to `lib`; `prefix` lets the tests bind the oracle twin (orc_*)."""
    for name, (res, args) in _PROTOTYPES.items():
        if names is not None and name not in names:
            continue
        fn = getattr(lib, prefix + name[len("ycge_"):])
        fn.restype = res
        fn.argtypes = args
    if prefix == "ycge_" and names is None:
        for name, (res, args) in HOOK_PROTOTYPES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
    return lib


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """Load libycge_hip.so.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path is not None else Path(os.environ.get("YCGE_LIB", LIB_PATH))
    if not p.exists():
        raise FileNotFoundError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the ray-trace path.")
    lib = bind(C.CDLL(str(p)))
    if path is None:
        _lib = lib
    return lib


def world_file_info(data, lib: C.CDLL | None = None):
    """ycge_world_file_info: the header of a VG01 file's bytes (no context, no device) -> ((nx, ny, nz), payload offset).  Raises YcgeError
    with the reference's text for what ReloadFromExistingFile refuses."""
    L = lib if lib is not None else load_library()
    fn = L.ycge_world_file_info
    fn.restype, fn.argtypes = _PROTOTYPES["ycge_world_file_info"]
    import numpy as np
    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else data
    dims, off, msg = (C.c_int32 * 3)(), C.c_size_t(0), C.create_string_buffer(256)
    rc = fn(buf.ctypes.data if buf.size else C.addressof(msg), buf.size, dims, C.byref(off), msg, len(msg))          # (an empty file is a short one, not a NULL argument)
    if rc != 0:
        raise YcgeError(rc, msg.value.decode())
    return tuple(int(v) for v in dims), int(off.value)


def mesh_ranges(ops, end0: int = 0, n_index0: int = 0, lib: C.CDLL | None = None):
    """ycge_debug_mesh_ranges: the mesh pool's allocator alone (no context, no device) run through `ops` - rows {op, a, b} with op one of
    MESH_RANGE_TAKE (a units), MESH_RANGE_GIVE (the b units at unit a), MESH_INDEX_TAKE, MESH_INDEX_GIVE (index a) -> int64 [n, 4]: per op
    {the take's answer, the records' end, free ranges, free units}."""
    import numpy as np
    L = lib if lib is not None else load_library()
    fn = L.ycge_debug_mesh_ranges
    fn.restype, fn.argtypes = MESH_POOL_HOOK_PROTOTYPES["ycge_debug_mesh_ranges"]
    ops = np.ascontiguousarray(ops, np.int64).reshape(-1, 3)
    out = np.zeros((len(ops), 4), np.int64)
    rc = fn(end0, n_index0, ops.ctypes.data, len(ops), out.ctypes.data)
    if rc != 0:
        raise YcgeError(rc, "ycge_debug_mesh_ranges refused the arguments")
    return out


def obj_parse_host(data: bytes, lib: C.CDLL | None = None):
    """ycge_obj_parse_host: the library's host parser alone (no context, no device) -> (positions f32 [nv, 3], faces i32 [nt, 3], ObjInfo).
    Raises YcgeError with the refusal's text."""
    import numpy as np
    L = lib if lib is not None else load_library()
    fn = L.ycge_obj_parse_host
    fn.restype, fn.argtypes = _PROTOTYPES["ycge_obj_parse_host"]
    data = bytes(data)
    info, msg = ObjInfo(), C.create_string_buffer(256)
    rc = fn(data, len(data), None, None, C.byref(info), msg, len(msg))
    if rc != 0:
        raise YcgeError(rc, msg.value.decode())
    pos = np.empty((info.n_positions, 3), np.float32)
    faces = np.empty((info.n_triangles, 3), np.int32)
    rc = fn(data, len(data), pos.ctypes.data, faces.ctypes.data, C.byref(info), msg, len(msg))
    if rc != 0:
        raise YcgeError(rc, msg.value.decode())
    return pos, faces, info


def obj_geometry(lib: C.CDLL | None = None) -> dict:
    """the OBJ kernels' geometry and the environment's knobs as the library reads them now (no device)"""
    L = lib if lib is not None else load_library()
    fn = L.ycge_debug_obj_stats
    fn.restype, fn.argtypes = OBJ_HOOK_PROTOTYPES["ycge_debug_obj_stats"]
    out = (C.c_int64 * 6)()
    fn(None, out)
    return dict(zip(("tile_bytes", "lines_per_workgroup", "line_cap", "device_min", "env_host"), (int(v) for v in out)))


def obj_ground_host(pos, faces, lib: C.CDLL | None = None) -> ObjGroundInfo:
    """ycge_obj_ground_host: the library's host tail alone (no context, no device) on positions f32 [nv, 3] and faces i32 [nt, 3].
    Raises YcgeError when it refuses the arrays."""
    import numpy as np
    L = lib if lib is not None else load_library()
    fn = L.ycge_obj_ground_host
    fn.restype, fn.argtypes = _PROTOTYPES["ycge_obj_ground_host"]
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    info = ObjGroundInfo()
    rc = fn(pos.ctypes.data, len(pos), faces.ctypes.data, len(faces), C.byref(info))
    if rc != 0:
        raise YcgeError(rc, "ycge_obj_ground_host refused the arrays")
    return info


def obj_ground_geometry(lib: C.CDLL | None = None) -> dict:
    """the auto-ground kernels' geometry and the environment's knobs as the library reads them now (no device)"""
    L = lib if lib is not None else load_library()
    fn = L.ycge_debug_obj_ground_stats
    fn.restype, fn.argtypes = OBJ_GROUND_HOOK_PROTOTYPES["ycge_debug_obj_ground_stats"]
    out = (C.c_int64 * 6)()
    fn(None, out)
    return dict(zip(("sum_chunk", "round_cap", "device_min_default", "device_min", "env_host"), (int(v) for v in out)))
