"""RaytraceRenderer — host-side mirror of the reference's render entry point.

Same surface as ConsoleGame/RayTracing/RaytraceRenderer.cs (ctor :74, Resize :110,
SetCamera :140, SetFov :150, TryFlipAndBlit :157), i.e. the IConsoleRenderer seam of
RaytraceEntity.cs:12-18, implemented by calls through the C-ABI (include/ycge.h) into
the gfx950 kernels.  No per-pixel work happens in Python and there is no CPU fallback:
constructing a renderer without the built library or without an MI355X raises.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Optional

import numpy as np

from . import abi
from .scene import FlatScene, Mesh, NeedsUpload, Scene, VolumeGrid, flatten, grid_record, material_record, mesh_record

NODE_DTYPE = np.dtype([("min", "<f4", 3), ("max", "<f4", 3), ("left", "<i4"), ("right", "<i4"), ("start", "<i4"), ("count", "<i4")])


class _PageLockedOwner:
    """Owns one ycge_alloc_host_buffer allocation; frees it when collected (after the last numpy view over it)."""

    def __init__(self, lib, address: int):
        self._lib, self.address = lib, address

    def __del__(self):
        try:
            if self.address:
                self._lib.ycge_free_host_buffer(C.c_void_p(self.address))
                self.address = 0
        except Exception:
            pass


CHEXEL_DTYPE = np.dtype([("ch", "<u2"), ("pad", "<u2"), ("fg", "<f4", 3), ("bg", "<f4", 3)])          # abi.Chexel as a numpy record, 28 bytes


class ConsoleLayer:
    """A Framebuffer of the console beside the raytrace one (Renderer/Framebuffer.cs) as ycge_console_set_layers takes it: `chars` (h, w)
    UTF-16 code units - or h strings of w BMP characters - with `fg` and `bg` (h, w, 3) float32 colours (one colour broadcasts), at
    console position (x, y).  A cell whose character is ' ' is transparent."""

    def __init__(self, chars, fg=(0.75, 0.75, 0.75), bg=(0.0, 0.0, 0.0), x: int = 0, y: int = 0):
        if len(chars) and isinstance(chars[0], str):
            chars = [[ord(ch) for ch in row] for row in chars]
        self.chars = np.ascontiguousarray(chars, dtype=np.uint16)
        if self.chars.ndim != 2 or self.chars.size == 0:
            raise ValueError("a layer's characters are an (h, w) array, both positive")
        self.h, self.w = self.chars.shape
        self.fg = np.ascontiguousarray(np.broadcast_to(np.asarray(fg, np.float32), (self.h, self.w, 3)))
        self.bg = np.ascontiguousarray(np.broadcast_to(np.asarray(bg, np.float32), (self.h, self.w, 3)))
        self.x, self.y = int(x), int(y)

    def cells(self) -> np.ndarray:
        """the layer's ycge_chexel array, row by row"""
        c = np.zeros(self.h * self.w, CHEXEL_DTYPE)
        c["ch"], c["fg"], c["bg"] = self.chars.ravel(), self.fg.reshape(-1, 3), self.bg.reshape(-1, 3)
        return c

    def as_struct(self) -> "abi.ConsoleLayer":
        self._cells = self.cells()          # (kept alive for the length of the call that reads it)
        return abi.ConsoleLayer(self.x, self.y, self.w, self.h, self._cells.ctypes.data_as(C.POINTER(abi.Chexel)))


class RaytraceRenderer:
    def __init__(self, scene: Scene | FlatScene, fb_width: int, fb_height: int, fovDeg: float = 45.0, superSample: int = 1, *,
                 cfg: Optional[abi.Config] = None, capture_debug: bool = False, count_work: bool = False, device: int = 0,
                 rank: int = 0, world_size: int = 1, slab_albedo: bool = True, devices=None, lib=None, tile_ring: int = 0):
        self.L = lib if lib is not None else abi.load_library()
        c = cfg if cfg is not None else abi.default_config()
        c.fb_width, c.fb_height, c.super_sample = fb_width, fb_height, max(1, superSample)
        c.fov_deg = fovDeg
        c.capture_debug, c.count_work = int(capture_debug), int(count_work)
        c.device, c.rank, c.world_size = device, rank, world_size
        c.tile_ring = int(tile_ring)              # tile-resident form: frame sets in the ring (0 = 2)
        c.slab_albedo = int(slab_albedo)          # tiled frame: lean 8-float slabs when the denoise stage will not run
        if devices is not None:                   # one process, several GPUs: TryFlipAndBlit drives them all (config.n_devices)
            c.n_devices = len(devices)
            for i, d in enumerate(devices):
                c.devices[i] = int(d)
        self.cfg = c
        self.ctx = C.c_void_p()
        rc = self.L.ycge_create(C.byref(c), C.byref(self.ctx))
        if rc != 0:
            raise abi.YcgeError(rc, (self.L.ycge_last_error(None) or b"").decode())
        self._set_dims(fb_width, fb_height, c.super_sample)
        self._pos, self._yaw, self._pitch, self._fov = (0.0, 1.0, 0.0), 0.0, 0.0, fovDeg
        self.flat = None
        self._streamed = {}          # id -> VolumeGrid attached by AttachGrids and still resident
        self._streamed_meshes = {}   # id -> Mesh attached by AttachMeshes and still resident
        self.stream_call_s = {"attach": 0.0, "update": 0.0, "detach": 0.0}          # seconds inside the last library call of each kind (profiles/stream_rate.py)
        self.stats = abi.FrameStats()
        if scene is not None:
            self.UploadScene(scene)          # the C# ctor ends with scene.RebuildBVH() (:107)

    # ---------------------------------------------------------------- plumbing
    def _set_dims(self, w, h, ss):
        self.fbW, self.fbH, self.ss = w, h, ss
        self.hiW, self.hiH = w * ss, h * 2 * ss

    def _check(self, rc: int):
        if rc != 0:
            raise abi.YcgeError(rc, (self.L.ycge_last_error(self.ctx) or b"").decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.L.ycge_destroy(self.ctx)          # (waits for the frames in flight: their SDR arrays are still the wrapper's)
            self.ctx = C.c_void_p()
        self._drop_sdr_buffer()
        self._drop_sdr_ring()
        self.__dict__.pop("_chexel_ring", None)          # (the chexel arrays of the frames in flight: after ycge_destroy, as above)
        self.__dict__.pop("_ansi_buf", None)             # (the page-locked stream buffer)
        self.__dict__.pop("_ansi_ring", None)            # (the stream buffers and records of the frames in flight)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- reference surface
    def UploadScene(self, scene: Scene | FlatScene):
        """scene.RebuildBVH() + upload (RaytraceRenderer.cs:107, RaytraceEntity.cs:244)."""
        self.flat = scene if hasattr(scene, "byref") else flatten(scene)          # (a FlatScene, or a scene file read back: tools/scene_file.py)
        self._streamed = {}          # (the next upload forgets every attached grid)
        self._streamed_meshes = {}   # (... and every attached mesh)
        self._check(self.L.ycge_scene_upload(self.ctx, self.flat.byref()))

    def UpdateLights(self, lights, ambient=None, background_top=None, background_bottom=None):
        arr = (abi.Light * max(1, len(lights)))()
        for i, l in enumerate(lights):
            arr[i].position, arr[i].color, arr[i].intensity = abi.Vec3(*l.Position), abi.Vec3(*l.Color), float(l.Intensity)
        amb = abi.Vec3(*ambient.Color) if ambient is not None else None
        top = abi.Vec3(*background_top) if background_top is not None else None
        bot = abi.Vec3(*background_bottom) if background_bottom is not None else None
        self._check(self.L.ycge_scene_update_lights(
            self.ctx, arr, len(lights), C.byref(amb) if amb is not None else None,
            float(ambient.Intensity) if ambient is not None else 0.0,
            C.byref(top) if top is not None else None, C.byref(bot) if bot is not None else None))

    def UpdateTexture(self, texture) -> None:
        """The next frame of a live texture (LiveTexture.set_frame before this call): what IFrameReader.GetCurrentFramePtr() returns
        while the coming frames are traced (Renderer/Texture.cs:116)."""
        idx = next(i for i, t in enumerate(self.flat.texture_objects) if t is texture)
        f = texture.frame
        self._check(self.L.ycge_scene_update_texture(self.ctx, idx, f.ctypes.data_as(C.c_void_p), f.nbytes))

    def UpdateObjects(self, scene: Scene | FlatScene):
        """Scene.Update() -> RebuildBVH() after entities moved (Scene.cs:122-127): same materials, meshes and grids
        as the uploaded scene (in the same first-use order), new object records; only the scene BVH is rebuilt."""
        f = scene if isinstance(scene, FlatScene) else flatten(scene, against=self.flat if hasattr(self.flat, "_mat_index") else None)          # (a Scene: numbered against the upload; NeedsUpload if it holds something new)
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_update_objects(self.ctx, C.cast(f.prims, C.POINTER(abi.Prim)), f.struct.n_prims)
        self.stream_call_s["update"] = time.perf_counter() - t0
        self._check(rc)
        self.flat = f

    # ---------------------------------------------------------------- chunk streaming (ycge_scene_attach_grids / ycge_scene_detach_grids)
    def _material_numbering(self, append_new: bool):
        """(mat_id, finish): mat_id numbers a Material against those the library holds - one it does not hold raises NeedsUpload, or, with
        append_new, takes the next index behind them; finish() then appends those, once the records that name them are made."""
        if not hasattr(self.flat, "_mat_index"):
            raise NeedsUpload("the uploaded scene was not flattened from a Scene: its materials cannot be matched")
        mat_index = self.flat._mat_index
        base, new, provisional = len(mat_index), [], {}

        def mat_id(m):
            if id(m) in mat_index:
                return mat_index[id(m)]
            if not append_new:
                raise NeedsUpload("a material the uploaded scene does not hold")
            if id(m) not in provisional:
                provisional[id(m)] = base + len(new)
                new.append(m)
            return provisional[id(m)]

        def finish():
            if new:
                first = self.AppendMaterials(new)
                assert first == base, (first, base)

        return mat_id, finish

    def AttachGrids(self, grids, append_new_materials: bool = False) -> list:
        """Makes the VolumeGrids resident beside those of the upload and returns their device indices; no object refers to them until
        the next UpdateObjects / StreamObjects.  Their materials must be materials the library holds (NeedsUpload otherwise) - or, with
        append_new_materials, the ones it does not hold are appended first (AppendMaterials), as the records of these grids name them."""
        grids = list(grids)
        if not grids:
            return []
        mat_id, append_new = self._material_numbering(append_new_materials)
        keep = []
        recs = (abi.Grid * len(grids))(*[grid_record(g, mat_id, keep) for g in grids])
        append_new()
        out = (C.c_int32 * len(grids))()
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_attach_grids(self.ctx, recs, len(grids), out)
        self.stream_call_s["attach"] = time.perf_counter() - t0          # (the library call alone: what a native host pays)
        self._check(rc)
        idx = [int(i) for i in out]
        for g, i in zip(grids, idx):
            self.flat._grid_index[id(g)] = i
            self._streamed[id(g)] = g          # (keeps the object, hence its id, alive while it is resident)
        return idx

    def GenerateGrids(self, world: abi.World, keys, proto: abi.Grid, want_cells: bool = False):
        """ycge_scene_generate_grids: WorldGenerator.GenerateChunkCells for the chunk keys [(cx, cy, cz), ...] on the device, attached like
        AttachGrids' grids.  `proto` supplies the lookup table, default material and wireframe settings (its materials index the uploaded
        scene's).  Returns the device indices (-1: an all-air chunk, no slot) and, with want_cells, the raw cells [n, S, S, S, 2] int32."""
        keys = np.ascontiguousarray(np.asarray(keys, np.int32).reshape(-1, 3))
        n, S = keys.shape[0], int(world.chunk_size)
        out = (C.c_int32 * max(1, n))(*([-7] * max(1, n)))
        cells = np.zeros((n, S, S, S, 2), np.int32) if want_cells else None
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_generate_grids(self.ctx, C.byref(world), keys.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(proto), out,
                                              cells.ctypes.data_as(C.POINTER(C.c_int32)) if want_cells else None)
        self.stream_call_s["generate"] = time.perf_counter() - t0
        self._check(rc)
        idx = [int(out[k]) for k in range(n)]
        return (idx, cells) if want_cells else idx

    def GenerateWorld(self, world: abi.World, chunks_x: int, chunks_z: int, proto: abi.Grid, origin=(0, 0), want_cells: bool = False):
        """ycge_scene_generate_world: WorldManager.GenerateAndSaveWorld for a window of chunks_x x world.chunks_y x chunks_z chunks whose column
        (0, 0) is block `origin` - the reference's pregenerated world at origin (0, 0) - made on the device and attached like AttachGrids'
        grids, chunk (cx, cy, cz) at world_min + c * S * voxel_size.  Returns the device indices as int32 [chunks_x, chunks_y, chunks_z] (-1: a
        chunk of nothing but Air, no slot) and, with want_cells, the whole world's cells [nx, ny, nz, 2] int32 (the VG01 payload)."""
        S, cy = int(world.chunk_size), int(world.chunks_y)
        n = chunks_x * cy * chunks_z
        out = np.full(max(1, n), -7, np.int32)
        cells = np.zeros((chunks_x * S, cy * S, chunks_z * S, 2), np.int32) if want_cells else None
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_generate_world(self.ctx, C.byref(world), chunks_x, chunks_z, int(origin[0]), int(origin[1]), C.byref(proto),
                                              out.ctypes.data_as(C.POINTER(C.c_int32)), cells.ctypes.data_as(C.POINTER(C.c_int32)) if want_cells else None)
        self.stream_call_s["generate_world"] = time.perf_counter() - t0
        self._check(rc)
        idx = out[:n].reshape(chunks_x, cy, chunks_z)
        return (idx, cells) if want_cells else idx

    def worldpregen_stats(self) -> dict:
        """The last GenerateWorld on the root device: anyLeaves passes (the last flips nothing) and, in microseconds, the field kernels, the
        anyLeaves pass loop (wall time: a launch, a stream synchronise and a 4-byte read-back per pass), the occupancy kernel with its read-back, the fill kernels."""
        out = (C.c_int64 * 5)()
        fn = self.L.ycge_debug_worldpregen_stats
        fn.restype, fn.argtypes = abi.WORLDGEN_HOOK_PROTOTYPES["ycge_debug_worldpregen_stats"]
        self._check(fn(self.ctx, out))
        return dict(zip(("any_leaves_passes", "fields_us", "any_leaves_us", "occupied_us", "fill_us"), (int(v) for v in out)))

    def worldgen_stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self.L.ycge_debug_worldgen_stats.restype, self.L.ycge_debug_worldgen_stats.argtypes = abi.WORLDGEN_HOOK_PROTOTYPES["ycge_debug_worldgen_stats"]
        self._check(self.L.ycge_debug_worldgen_stats(self.ctx, out))
        return dict(zip(("device_chunks", "host_chunks", "last_columns_us", "last_fill_us"), (int(v) for v in out)))

    # ---------------------------------------------------------------- the world store (ycge_world_store_load / ycge_scene_attach_world_chunks)
    def LoadWorld(self, cells_or_path, chunk_size: int):
        """ycge_world_store_load: a VG01 world made resident on the device, once.  `cells_or_path` is the cells int32 [nx, ny, nz, 2] or the
        path of a VG01 file, which is mapped and handed over without a copy (its header checked by ycge_world_file_info).  Replaces a store
        the renderer holds; the scene is not touched.  Returns (nx, ny, nz)."""
        if isinstance(cells_or_path, np.ndarray):
            cells = np.ascontiguousarray(cells_or_path, np.int32)
            if cells.ndim != 4 or cells.shape[3] != 2:
                raise ValueError("cells must be [nx, ny, nz, 2]")
            dims = cells.shape[:3]
        else:
            if cells_or_path is None or str(cells_or_path).strip() == "":
                raise ValueError("filename is null or empty.")
            data = np.memmap(cells_or_path, np.uint8, "r")
            dims, off = abi.world_file_info(data, self.L)
            cells = data[off:off + 8 * dims[0] * dims[1] * dims[2]].view("<i4")
        t0 = time.perf_counter()
        rc = self.L.ycge_world_store_load(self.ctx, cells.ctypes.data, int(dims[0]), int(dims[1]), int(dims[2]), int(chunk_size))
        self.stream_call_s["load_world"] = time.perf_counter() - t0
        self._check(rc)
        return tuple(int(v) for v in dims)

    def GenerateWorldStore(self, world: abi.World, chunks_x: int, chunks_z: int, origin=(0, 0), form="fields"):
        """ycge_world_store_generate: the window of GenerateWorld made the renderer's world store on the device - GenerateAndSaveWorld and
        ReloadFromExistingFile in one call, with no cell on the bus.  form "fields": the window's 2-D fields stay resident and a chunk's cells
        are made when its key is attached; "cells": the ordinary cell store, written on the device.  Replaces a store the renderer holds;
        the scene is not touched.  Returns (nx, ny, nz)."""
        if form not in abi.WORLD_STORE_FORMS and not isinstance(form, int):
            raise ValueError("form must be 'fields' or 'cells'")
        t0 = time.perf_counter()
        rc = self.L.ycge_world_store_generate(self.ctx, C.byref(world) if world is not None else None, int(chunks_x), int(chunks_z), int(origin[0]), int(origin[1]),
                                              abi.WORLD_STORE_FORMS.get(form, form))
        self.stream_call_s["generate_world_store"] = time.perf_counter() - t0
        self._check(rc)
        S = int(world.chunk_size)
        return (chunks_x * S, int(world.chunks_y) * S, chunks_z * S)

    def ReadWorldCells(self, x0: int = 0, planes=None, out: np.ndarray | None = None) -> np.ndarray:
        """ycge_world_store_read: the x-planes [x0, x0 + planes) of the store (planes None: to the end) as int32 [planes, ny, nz, 2], VG01
        payload order - whatever the store is made of.  `out`, when given, is a C-contiguous int32 array of that size that receives them
        (a page-locked one is copied into directly)."""
        dims, S = (C.c_int32 * 3)(), C.c_int32(0)
        self._check(self.L.ycge_world_store_info(self.ctx, dims, C.byref(S), None, 0))
        if planes is None:
            planes = int(dims[0]) - int(x0)
        shape = (max(int(planes), 0), int(dims[1]), int(dims[2]), 2)
        if out is None:
            out = np.empty(shape, np.int32)
        elif out.dtype != np.int32 or not out.flags.c_contiguous or out.size != int(np.prod(shape)):
            raise ValueError("out must be C-contiguous int32 of planes * ny * nz * 2 elements")
        t0 = time.perf_counter()
        rc = self.L.ycge_world_store_read(self.ctx, int(x0), int(planes), out.ctypes.data)
        self.stream_call_s["read_world"] = time.perf_counter() - t0
        self._check(rc)
        return out.reshape(shape)

    def world_store_generate_stats(self) -> dict:
        """The last GenerateWorldStore on the root device: the form asked for, whether the host generator made the cells (the knobs), the
        anyLeaves passes (the last flips nothing), the slabs of k_wp_planes and, in microseconds, the field kernels, the anyLeaves pass loop
        (wall time), the occupancy kernel with its read-back, the plane kernels (stream time), the host generator."""
        fn = self.L.ycge_debug_world_store_generate_stats
        fn.restype, fn.argtypes = abi.WORLD_STORE_HOOK_PROTOTYPES["ycge_debug_world_store_generate_stats"]
        out = (C.c_int64 * 9)()
        self._check(fn(self.ctx, out))
        return dict(zip(abi.WORLD_STORE_GENERATE_STATS, (int(v) for v in out)))

    def WorldInfo(self):
        """ycge_world_store_info -> ((nx, ny, nz), chunk_size, occupied uint8 [chunks_x, chunks_y, chunks_z]: 1 where a cell has mat != 0)"""
        dims, S = (C.c_int32 * 3)(), C.c_int32(0)
        self._check(self.L.ycge_world_store_info(self.ctx, dims, C.byref(S), None, 0))
        counts = tuple(-(-int(d) // S.value) for d in dims)
        occ = np.zeros(counts, np.uint8)
        self._check(self.L.ycge_world_store_info(self.ctx, dims, C.byref(S), occ.ctypes.data, occ.size))
        return tuple(int(d) for d in dims), int(S.value), occ

    def AttachWorldChunks(self, keys, proto: abi.Grid) -> list:
        """ycge_scene_attach_world_chunks: the chunks [(cx, cy, cz), ...] of the store attached like AttachGrids' grids, sliced on the device.
        proto.min_corner is WorldMin and proto.voxel_size VoxelSize; its lookup table, default material and wireframe settings serve every
        chunk.  Returns the device indices; -1 for a key outside the world and for a chunk with no cell of mat != 0 (no slot)."""
        keys = np.ascontiguousarray(np.asarray(keys, np.int32).reshape(-1, 3))
        n = keys.shape[0]
        out = (C.c_int32 * max(1, n))(*([-7] * max(1, n)))
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_attach_world_chunks(self.ctx, keys.ctypes.data_as(C.POINTER(C.c_int32)), n, C.byref(proto), out)
        self.stream_call_s["attach_world"] = time.perf_counter() - t0
        self._check(rc)
        return [int(out[k]) for k in range(n)]

    # ---------------------------------------------------------------- voxel edits (ycge_scene_edit_voxels / ycge_world_store_edit)
    @staticmethod
    def _edit_ops(ops) -> np.ndarray:
        """int32 [n, 9] = ycge_voxel_edit: {grid_index, lo xyz, hi xyz, mat_id, meta_id} per op (rows of nine, or (grid, lo, hi, mat, meta))."""
        rows = [np.concatenate([np.atleast_1d(np.asarray(f, np.int64)).ravel() for f in op]) for op in ops] if not isinstance(ops, np.ndarray) else ops
        arr = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 9)).astype(np.int32)
        assert arr.itemsize * 9 == C.sizeof(abi.VoxelEdit)
        return arr

    def EditVoxels(self, ops) -> dict:
        """ycge_scene_edit_voxels: every cell of each op's inclusive box lo..hi of resident grid grid_index becomes (mat_id, meta_id), in list
        order (where boxes overlap the later op wins).  The scene is complete afterwards - the objects are installed again when a held
        grid's solid box or brick mask changed.  All or nothing: a refused list (YcgeError, the message names the op) changes nothing.
        Returns {cells_changed, bricks_written, records_changed, objects_installed}."""
        arr = self._edit_ops(ops)
        info = (C.c_uint32 * 4)()
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_edit_voxels(self.ctx, arr.ctypes.data if len(arr) else None, len(arr), info)
        self.stream_call_s["edit"] = time.perf_counter() - t0
        self._check(rc)
        return dict(zip(abi.VOXEL_EDIT_INFO, (int(v) for v in info)))

    def EditWorldCells(self, ops) -> None:
        """ycge_world_store_edit: the same ops in store cell coordinates (grid_index 0) written into the world store as raw pairs; the
        occupancy of the chunks they touch follows.  No scene is touched: grids attached earlier keep their cells (EditVoxels)."""
        arr = self._edit_ops(ops)
        t0 = time.perf_counter()
        rc = self.L.ycge_world_store_edit(self.ctx, arr.ctypes.data if len(arr) else None, len(arr))
        self.stream_call_s["edit_world"] = time.perf_counter() - t0
        self._check(rc)

    def ReserveWorldEdits(self, max_chunks: int) -> None:
        """ycge_world_store_reserve_edits: a pool of max_chunks materialised chunks (chunk_size^3 * 8 bytes each, on every device) beside a
        fields store, so EditWorldCells works on it: every chunk an op touches takes a slot until RevertWorldChunks gives it back."""
        self._check(self.L.ycge_world_store_reserve_edits(self.ctx, int(max_chunks)))

    def WorldEditSlots(self):
        """ycge_world_store_edit_slots -> (slots of the pool, slots that hold a chunk); (0, 0) without a pool"""
        cap, used = C.c_int32(-1), C.c_int32(-1)
        self._check(self.L.ycge_world_store_edit_slots(self.ctx, C.byref(cap), C.byref(used)))
        return cap.value, used.value

    def RevertWorldChunks(self, keys) -> None:
        """ycge_world_store_revert_chunks: these chunks (cx, cy, cz) give their slots back and are the generated chunks again"""
        k = np.ascontiguousarray(np.asarray(keys, np.int32).reshape(-1, 3))
        self._check(self.L.ycge_world_store_revert_chunks(self.ctx, k.ctypes.data_as(C.POINTER(C.c_int32)) if len(k) else None, len(k)))

    def ReleaseWorld(self) -> None:
        self._check(self.L.ycge_world_store_release(self.ctx))

    def world_store_chunk(self, cx: int, cy: int, cz: int) -> np.ndarray:
        """One chunk's raw cells [sx, sy, sz, 2] as the slice writes them (ycge_debug_world_store_chunk); no attach."""
        fn = self.L.ycge_debug_world_store_chunk
        fn.restype, fn.argtypes = abi.WORLD_STORE_HOOK_PROTOTYPES["ycge_debug_world_store_chunk"]
        dims = (C.c_int32 * 3)()
        self._check(fn(self.ctx, cx, cy, cz, None, dims))
        cells = np.zeros((dims[0], dims[1], dims[2], 2), np.int32)
        self._check(fn(self.ctx, cx, cy, cz, cells.ctypes.data, dims))
        return cells

    def world_store_stats(self) -> dict:
        """The store's bytes, the last load's slabs and split in microseconds (copies into the staging: wall; host-to-device copies and
        occupancy kernels: stream time, they overlap), the last AttachWorldChunks' slice kernels, chunks sliced on the device / the host."""
        fn = self.L.ycge_debug_world_store_stats
        fn.restype, fn.argtypes = abi.WORLD_STORE_HOOK_PROTOTYPES["ycge_debug_world_store_stats"]
        out = (C.c_int64 * 8)()
        self._check(fn(self.ctx, out))
        st = dict(zip(abi.WORLD_STORE_STATS, (int(v) for v in out)))
        # the pool of materialised chunks beside a fields store: its slots, those in use, its bytes on one device (not part of store_bytes)
        st["edit_slots"], st["edit_slots_used"] = self.WorldEditSlots()
        st["edit_pool_bytes"] = 0
        if st["edit_slots"]:
            S = C.c_int32(0)
            self._check(self.L.ycge_world_store_info(self.ctx, None, C.byref(S), None, 0))
            st["edit_pool_bytes"] = st["edit_slots"] * S.value ** 3 * 8
        return st

    # ---------------------------------------------------------------- OBJ meshes from file bytes (MeshLoader.FromObj on the device)
    def ParseObj(self, data) -> abi.ObjInfo:
        """ycge_obj_parse: `data` is the file's bytes or a path.  The context holds the parsed OBJ until the next ParseObj, ReleaseObj or close."""
        if not isinstance(data, (bytes, bytearray, memoryview)):
            with open(data, "rb") as fh:
                data = fh.read()
        data = bytes(data)
        info = abi.ObjInfo()
        self._check(self.L.ycge_obj_parse(self.ctx, data, len(data), C.byref(info)))
        self._obj_info = info
        return info

    def ReadObj(self):
        """ycge_obj_read -> (positions f32 [nv, 3], faces i32 [nt, 3]) of the held OBJ"""
        info = getattr(self, "_obj_info", None)
        pos = np.empty((info.n_positions if info else 0, 3), np.float32)
        faces = np.empty((info.n_triangles if info else 0, 3), np.int32)
        self._check(self.L.ycge_obj_read(self.ctx, pos.ctypes.data if info else None, faces.ctypes.data if info else None))
        return pos, faces

    def ObjTriangles(self, scale: float = 1.0, translate=(0.0, 0.0, 0.0), normalize: bool = True, target_size: float = 1.0):
        """ycge_obj_triangles: MeshLoader.FromObj's tail for the held OBJ -> (triangles f32 [nt, 3, 3], bounds f32 [6] = min xyz, max xyz)"""
        info = getattr(self, "_obj_info", None)
        tris = np.empty((info.n_triangles if info else 0, 3, 3), np.float32)
        bounds = np.empty(6, np.float32)
        t = (C.c_float * 3)(*[float(np.float32(v)) for v in translate])
        self._check(self.L.ycge_obj_triangles(self.ctx, int(bool(normalize)), float(np.float32(target_size)), float(np.float32(scale)), t,
                                               tris.ctypes.data if info else None, bounds.ctypes.data))
        return tris, bounds

    def ObjGround(self) -> abi.ObjGroundInfo:
        """ycge_obj_ground: MeshScenes.TryReadObjBoundsNormalized behind its parse, for the held OBJ - the component with the most faces, its
        centroid, the normalised bounds of its vertices about it; info.on_device says whether the kernels ran it."""
        info = abi.ObjGroundInfo()
        self._check(self.L.ycge_obj_ground(self.ctx, C.byref(info)))
        return info

    def ObjTrianglesAutoGround(self, scale: float, target_pos):
        """ycge_obj_triangles_auto_ground: MeshScenes.AddMeshAutoGround for the held OBJ in one call -> (triangles f32 [nt, 3, 3], bounds f32
        [6] = min xyz, max xyz, ObjGroundInfo)"""
        info = getattr(self, "_obj_info", None)
        tris = np.empty((info.n_triangles if info else 0, 3, 3), np.float32)
        bounds = np.empty(6, np.float32)
        ground = abi.ObjGroundInfo()
        t = (C.c_float * 3)(*[float(np.float32(v)) for v in target_pos])
        self._check(self.L.ycge_obj_triangles_auto_ground(self.ctx, float(np.float32(scale)), t, tris.ctypes.data if info else None, bounds.ctypes.data, C.byref(ground)))
        return tris, bounds, ground

    def ReleaseObj(self) -> None:
        self._obj_info = None
        self._check(self.L.ycge_obj_release(self.ctx))

    def obj_stats(self) -> dict:
        """Who parsed: files the kernels parsed, files the host parser took, why the last one went to the host (abi.OBJ_DECLINE_*; 0: it did
        not), wall microseconds of the last parse's line passes, of its token and index passes, of the last ObjTriangles' pass."""
        out = (C.c_int64 * 6)()
        fn = self.L.ycge_debug_obj_stats
        fn.restype, fn.argtypes = abi.OBJ_HOOK_PROTOTYPES["ycge_debug_obj_stats"]
        self._check(fn(self.ctx, out))
        return dict(zip(abi.OBJ_STATS, (int(v) for v in out)))

    def obj_ground_stats(self) -> dict:
        """Who ran the auto-ground tail: tails the kernels ran, tails the host ran, why the last one went to the host (abi.OBJ_GROUND_DECLINE_*;
        0: it did not), the labelling rounds of the last device tail, sums that fell back to a serial path (no chunked sum is built: 0), wall
        microseconds of the last tail; with YCGE_OBJ_GROUND_PHASES set at creation also the last device tail's phases (abi.OBJ_GROUND_PHASES)."""
        out = (C.c_int64 * 6)()
        fn = self.L.ycge_debug_obj_ground_stats
        fn.restype, fn.argtypes = abi.OBJ_GROUND_HOOK_PROTOTYPES["ycge_debug_obj_ground_stats"]
        self._check(fn(self.ctx, out))
        d = dict(zip(abi.OBJ_GROUND_STATS, (int(v) for v in out)))
        ph = (C.c_int64 * 5)()
        fn = self.L.ycge_debug_obj_ground_phases
        fn.restype, fn.argtypes = abi.OBJ_GROUND_HOOK_PROTOTYPES["ycge_debug_obj_ground_phases"]
        self._check(fn(self.ctx, ph))
        d.update(zip(abi.OBJ_GROUND_PHASES, (int(v) for v in ph)))
        return d

    def DetachGrids(self, indices) -> None:
        """Gives the grids' slots back; refused while Scene.Objects (as of the last UpdateObjects) refer to one of them."""
        indices = [int(i) for i in indices]
        if not indices:
            return
        arr = (C.c_int32 * len(indices))(*indices)
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_detach_grids(self.ctx, arr, len(indices))
        self.stream_call_s["detach"] = time.perf_counter() - t0
        self._check(rc)
        gone = set(indices)
        for key in [k for k, i in self.flat._grid_index.items() if i in gone]:
            del self.flat._grid_index[key]
            self._streamed.pop(key, None)

    def StreamObjects(self, scene: Scene, keep_cached: bool = False):
        """The Scene.Update that follows WorldManager.LoadChunksAround: the scene's VolumeGrid objects (by identity) against the resident
        ones - attach the new, UpdateObjects with the references mapped to device indices, detach what no longer appears (or keep it
        resident and unreferenced when keep_cached: the reference's chunk cache).  Returns (attached indices, detached indices).
        Mesh objects are streamed the same way, and Materials the library does not hold yet are appended first - those of the analytic
        objects, and those the records of the NEW grids and meshes name; a resident grid or mesh is not looked at again (a texture the upload
        did not hold still raises NeedsUpload); what was attached and detached of them: self.streamed_meshes = (attached, detached)."""
        resident = self.flat._grid_index
        resident_meshes = self.flat._mesh_index
        self.stream_call_s.update(attach=0.0, update=0.0, detach=0.0, attach_meshes=0.0, detach_meshes=0.0)
        new_mats = self._analytic_materials_not_held(scene)
        if new_mats:
            self.AppendMaterials(new_mats)
        wanted = [o for o in scene.Objects if isinstance(o, VolumeGrid)]
        wanted_meshes = [o for o in scene.Objects if isinstance(o, Mesh)]
        attached = self.AttachGrids([o for o in wanted if id(o) not in resident], append_new_materials=True)
        new_meshes, seen = [], set()
        for o in wanted_meshes:
            if id(o) not in resident_meshes and id(o) not in seen:
                seen.add(id(o)); new_meshes.append(o)
        attached_meshes = self.AttachMeshes(new_meshes, append_new_materials=True)
        self.UpdateObjects(scene)
        detached, detached_meshes = [], []
        if not keep_cached:
            live = {id(o) for o in wanted}
            detached = sorted(i for k, i in resident.items() if k not in live)
            self.DetachGrids(detached)
            live = {id(o) for o in wanted_meshes}
            detached_meshes = sorted(i for k, i in resident_meshes.items() if k not in live)
            self.DetachMeshes(detached_meshes)
        self.streamed_meshes = (attached_meshes, detached_meshes)
        return attached, detached

    def _analytic_materials_not_held(self, scene: Scene) -> list:
        """the Materials of the scene's analytic objects the library does not hold yet, in first-use order (grids and meshes: their
        records name what they need when they are attached - a resident one is not looked at again)"""
        held = getattr(self.flat, "_mat_index", None)
        if held is None:
            return []
        out, seen = [], set()
        for o in scene.Objects:
            if isinstance(o, (VolumeGrid, Mesh)):
                continue
            for m in (getattr(o, "Mat", None), getattr(o, "MaterialFunc", None)):
                if m is not None and id(m) not in held and id(m) not in seen:
                    seen.add(id(m)); out.append(m)
        return out

    # ---------------------------------------------------------------- meshes and materials of a resident scene (ycge_scene_attach_meshes / _detach_meshes / _append_materials)
    def AppendMaterials(self, materials) -> int:
        """New Materials behind those of the uploaded scene; returns the first new index (and numbers them in flat._mat_index).  A textured
        one must use a texture of the uploaded scene (NeedsUpload otherwise).  The next UpdateObjects / StreamObjects publishes what the
        longer list changes (a transparent, textured or mirroring material)."""
        materials = list(materials)
        if not hasattr(self.flat, "_mat_index"):
            raise NeedsUpload("the uploaded scene was not flattened from a Scene: its materials cannot be matched")
        if not materials:
            return len(self.flat._mat_index)

        def texture_id(t) -> int:
            for i, have in enumerate(self.flat.texture_objects):
                if have is t:
                    return i
            raise NeedsUpload("a texture the uploaded scene does not hold")

        recs = (abi.Material * len(materials))(*[material_record(m, texture_id) for m in materials])
        first = C.c_int32(-1)
        self._check(self.L.ycge_scene_append_materials(self.ctx, recs, len(materials), C.byref(first)))
        for k, m in enumerate(materials):
            self.flat._mat_index[id(m)] = first.value + k
            self.flat._keep.append(m)          # (keeps the object, hence its id, alive)
        return int(first.value)

    def AttachMeshes(self, meshes, append_new_materials: bool = False) -> list:
        """Makes the Meshes resident beside those of the upload and returns their device indices; no object refers to them until the next
        UpdateObjects / StreamObjects.  Their materials must be materials the library holds (the upload's, AppendMaterials'; NeedsUpload
        otherwise) - or, with append_new_materials, the ones it does not hold are appended first, as the records of these meshes name them."""
        meshes = list(meshes)
        if not meshes:
            return []
        mat_id, append_new = self._material_numbering(append_new_materials)
        keep = []
        recs = (abi.Mesh * len(meshes))(*[mesh_record(o, mat_id, keep) for o in meshes])
        append_new()
        out = (C.c_int32 * len(meshes))()
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_attach_meshes(self.ctx, recs, len(meshes), out)
        self.stream_call_s["attach_meshes"] = time.perf_counter() - t0
        self._check(rc)
        idx = [int(i) for i in out]
        for o, i in zip(meshes, idx):
            self.flat._mesh_index[id(o)] = i
            self._streamed_meshes[id(o)] = o          # (keeps the object, hence its id, alive while it is resident)
        return idx

    def DetachMeshes(self, indices) -> None:
        """Gives the meshes' indices and records back; refused while Scene.Objects (as of the last UpdateObjects) refer to one of them."""
        indices = [int(i) for i in indices]
        if not indices:
            return
        arr = (C.c_int32 * len(indices))(*indices)
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_detach_meshes(self.ctx, arr, len(indices))
        self.stream_call_s["detach_meshes"] = time.perf_counter() - t0
        self._check(rc)
        gone = set(indices)
        for key in [k for k, i in self.flat._mesh_index.items() if i in gone]:
            del self.flat._mesh_index[key]
            self._streamed_meshes.pop(key, None)

    def AttachObjMesh(self, material, scale: float = 1.0, translate=(0.0, 0.0, 0.0), normalize: bool = True, target_size: float = 1.0, auto_ground: bool = False,
                      target_pos=None):
        """ycge_scene_attach_obj_mesh: the held OBJ placed as ObjTriangles (or, with auto_ground, as ObjTrianglesAutoGround at target_pos)
        places it becomes a resident mesh of `material` (a Material the library holds, or its index) without its triangles crossing the
        bus -> (device index, bounds f32 [6])."""
        mi = material if isinstance(material, int) else self.flat._mat_index.get(id(material))
        if mi is None:
            raise NeedsUpload("a material the uploaded scene does not hold")
        t = (C.c_float * 3)(*[float(np.float32(v)) for v in (target_pos if auto_ground else translate)])
        out, bounds = C.c_int32(-1), np.empty(6, np.float32)
        t0 = time.perf_counter()
        rc = self.L.ycge_scene_attach_obj_mesh(self.ctx, int(bool(auto_ground)), int(bool(normalize)), float(np.float32(target_size)), float(np.float32(scale)), t, int(mi),
                                               C.byref(out), bounds.ctypes.data)
        self.stream_call_s["attach_meshes"] = time.perf_counter() - t0
        self._check(rc)
        return int(out.value), bounds

    def mesh_pool_stats(self) -> dict:
        """The pool of resident meshes (ycge_debug_mesh_pool_stats) and the last attach's host-side split in microseconds."""
        out = (C.c_int64 * 12)()
        fn = self.L.ycge_debug_mesh_pool_stats
        fn.restype, fn.argtypes = abi.MESH_POOL_HOOK_PROTOTYPES["ycge_debug_mesh_pool_stats"]
        self._check(fn(self.ctx, out))
        return {k: int(v) for k, v in zip(abi.MESH_POOL_STATS, out)}

    def grid_pool_stats(self) -> dict:
        """The pool of resident grids (ycge_debug_grid_pool_stats) and the last attach's host-side split in microseconds."""
        out = (C.c_int64 * 12)()
        self._check(self.L.ycge_debug_grid_pool_stats(self.ctx, out))
        keys = ("resident", "free_indices", "arena_in_use", "arena_capacity", "arena_growths", "slots_reused", "device_encodes", "host_encodes",
                "last_stage_us", "last_h2d_us", "last_kernel_us", "last_readback_us")
        return {k: int(v) for k, v in zip(keys, out)}

    def read_grid(self, index: int, shape):
        """A resident grid as the device holds it (ycge_debug_read_grid): (record bytes, int32 material per voxel [nx, ny, nz], -1 = empty)."""
        rec = np.zeros(abi.GGRID_BYTES, np.uint8)
        mats = np.zeros(tuple(shape), np.int32)
        self._check(self.L.ycge_debug_read_grid(self.ctx, int(index), rec.ctypes.data_as(C.c_void_p), mats.ctypes.data_as(C.c_void_p)))
        return rec, mats

    # ---------------------------------------------------------------- scene queries (ycge_scene_hit / ycge_scene_occluded)
    @staticmethod
    def _query_rays(origins, dirs, t_min, t_max) -> np.ndarray:
        """n x 8 f32 {o, d, tmin, tmax}; t_min / t_max may be scalars (broadcast) or length-n arrays."""
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"origins {o.shape} and dirs {d.shape} differ")
        rays = np.empty((o.shape[0], 8), dtype=np.float32)
        rays[:, 0:3], rays[:, 3:6] = o, d
        rays[:, 6] = np.broadcast_to(np.asarray(t_min, dtype=np.float32), (o.shape[0],))
        rays[:, 7] = np.broadcast_to(np.asarray(t_max, dtype=np.float32), (o.shape[0],))
        return rays

    def Hit(self, origins, dirs, t_min=0.001, t_max=np.float32(3.4028234663852886e38)):
        """Scene.Hit (Scene.cs:71-75) for n rays against the uploaded scene: (hits[n, 10] f32 {t, p xyz, n xyz, albedo rgb},
        ids[n, 2] i32 {Scene.Objects index, sub}); a miss is ids (-1, -1) and a zero record.  Runs beside frames in flight."""
        rays = self._query_rays(origins, dirs, t_min, t_max)
        n = rays.shape[0]
        hits = np.zeros((n, 10), dtype=np.float32)
        ids = np.zeros((n, 2), dtype=np.int32)
        self._check(self.L.ycge_scene_hit(self.ctx, rays.ctypes.data_as(C.POINTER(C.c_float)), n,
                                          hits.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data_as(C.POINTER(C.c_int32))))
        return hits, ids

    def Occluded(self, origins, dirs, t_min=0.001, t_max=np.float32(3.4028234663852886e38)) -> np.ndarray:
        """Scene.Occluded / the boolean of Scene.Hit for n rays: bool[n]."""
        rays = self._query_rays(origins, dirs, t_min, t_max)
        n = rays.shape[0]
        out = np.zeros(n, dtype=np.uint8)
        self._check(self.L.ycge_scene_occluded(self.ctx, rays.ctypes.data_as(C.POINTER(C.c_float)), n, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    # ---------------------------------------------------------------- the camera tick (ycge_volume_camera_tick)
    def CameraTick(self, body: "abi.CameraBody", world: "abi.CameraWorld", moves, dt_ms: float, run_update: bool = True) -> dict:
        """VolumeScene.HandleInput's moves, then VolumeScene.Update's physics (Scenes/VolumeScenes.cs:51-159, :165-530), in one launch on the
        device scene: `body` is updated in place on success and the counters of ycge_camera_tick_info come back.  moves: abi.CameraMove
        records (or (kind, shift, a, b) tuples) in the order received.  A refusal or a reached cap raises YcgeError and leaves body as it
        was.  Runs beside frames in flight, as Hit does."""
        recs = (abi.CameraMove * max(1, len(moves)))()
        for i, m in enumerate(moves):
            recs[i] = m if isinstance(m, abi.CameraMove) else abi.CameraMove(int(m[0]), int(m[1]), float(m[2]), float(m[3]))
        info = abi.CameraTickInfo()
        self._check(self.L.ycge_volume_camera_tick(self.ctx, C.byref(body), C.byref(world), recs if len(moves) else None, len(moves), float(dt_ms),
                                                   1 if run_update else 0, C.byref(info)))
        return {n: int(getattr(info, n)) for n, _ in abi.CameraTickInfo._fields_ if n != "reserved"}

    # ---------------------------------------------------------------- many bodies a tick (ycge_volume_bodies_tick)
    def BodiesTick(self, bodies, world: "abi.CameraWorld", moves, dt_ms: float, run_update: bool = True, shapes=None):
        """n independent bodies a tick in one launch: `bodies` is a ctypes array of abi.CameraBody (updated in place, body by body, where the
        tick committed), `moves` one list of move records (abi.CameraMove or (kind, shift, a, b) tuples) per body, `shapes` a ctypes array
        of abi.BodyShape or None for the reference's sizes.  Returns (results, infos): per body (status, bad_move) - 0 committed, 1 / 2 a
        horizontal / vertical move reached the micro-step cap, 3 the position stopped being finite, the body then left as it was - and the
        counters of ycge_camera_tick_info.  A refusal raises YcgeError and writes nothing.  Runs beside frames in flight, as Hit does."""
        n = len(bodies)
        if len(moves) != n or (shapes is not None and len(shapes) != n):
            raise ValueError("BodiesTick: one list of moves (and one shape) per body")
        first = (C.c_int32 * (n + 1))()
        flat = []
        for i, ms in enumerate(moves):
            flat.extend(m if isinstance(m, abi.CameraMove) else abi.CameraMove(int(m[0]), int(m[1]), float(m[2]), float(m[3])) for m in ms)
            first[i + 1] = len(flat)
        recs = (abi.CameraMove * max(1, len(flat)))(*flat)
        results = (abi.BodyResult * max(1, n))()
        info = (abi.CameraTickInfo * max(1, n))()
        self._check(self.L.ycge_volume_bodies_tick(self.ctx, C.byref(bodies) if n else None, C.byref(shapes) if shapes is not None and n else None, n,
                                                   C.byref(world), recs if flat else None, first, float(dt_ms), 1 if run_update else 0, results, info))
        names = [f for f, _ in abi.CameraTickInfo._fields_ if f != "reserved"]
        return ([(int(results[i].status), int(results[i].bad_move)) for i in range(n)],
                [{f: int(getattr(info[i], f)) for f in names} for i in range(n)])

    def scene_bvh_stats(self) -> dict:
        """How ycge_scene_update_objects built the scene BVH so far: on the device (csrc/ycge_bvh_build.hip), on the host after the
        kernel declined, on the host outright; microseconds of the last build + install; how often the current tree took the
        reference's Array.Sort path (BVH.cs:389,419) and its depth."""
        out = (C.c_int64 * 6)()
        self.L.ycge_debug_scene_bvh_stats.restype = C.c_int
        self.L.ycge_debug_scene_bvh_stats.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.L.ycge_debug_scene_bvh_stats(self.ctx, out))
        return dict(device_builds=int(out[0]), host_fallbacks=int(out[1]), host_builds=int(out[2]), last_build_us=int(out[3]),
                    sort_fallbacks=int(out[4]), max_depth=int(out[5]))

    def mesh_bvh_stats(self) -> dict:
        """How ycge_scene_upload built the mesh BVHs: on the device (csrc/ycge_mesh_bvh_build.hip), on the host, on the host after the device
        builder declined (counted as host builds too) - since the context was made; microseconds of the last device build (items kernel to
        the tree in host memory); and of the last upload: Array.Sort cases, deepest tree, wide nodes, subtree workgroups."""
        out = (C.c_int64 * 8)()
        fn = self.L.ycge_debug_mesh_bvh_stats
        fn.restype, fn.argtypes = abi.MESH_BVH_HOOK_PROTOTYPES["ycge_debug_mesh_bvh_stats"]
        self._check(fn(self.ctx, out))
        return {k: int(v) for k, v in zip(abi.MESH_BVH_STATS, out)}

    def mesh_emit_stats(self) -> dict:
        """Who wrote the mesh arena of the last ycge_scene_upload: meshes whose records the device wrote (csrc/ycge_mesh_emit.hip: an upload with
        at least one tree built on the device), meshes whose records the host wrote, microseconds of the device's layout + records + treelets,
        the arena's bytes."""
        out = (C.c_int64 * 4)()
        fn = self.L.ycge_debug_mesh_emit_stats
        fn.restype, fn.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_mesh_emit_stats"]
        self._check(fn(self.ctx, out))
        return {k: int(v) for k, v in zip(abi.MESH_EMIT_STATS, out)}

    def read_mesh_arena(self):
        """(bytes, tl_offset): the mesh arena the device holds - records, then the treelet region (0: none) - whichever side wrote it."""
        fn = self.L.ycge_debug_read_mesh_arena
        fn.restype, fn.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_read_mesh_arena"]
        tl = C.c_uint32(0)
        n = fn(self.ctx, None, 0, C.byref(tl))
        self._check(min(n, 0))
        out = np.zeros(max(n, 1), np.uint8)
        self._check(min(fn(self.ctx, out.ctypes.data, n, C.byref(tl)), 0))
        return out[:n], int(tl.value)

    def read_meshes(self) -> np.ndarray:
        """The GMesh records the device holds, [n, 8] uint32: root box (min xyz, max xyz), root reference, padding."""
        fn = self.L.ycge_debug_read_meshes
        fn.restype, fn.argtypes = abi.MESH_EMIT_HOOK_PROTOTYPES["ycge_debug_read_meshes"]
        n = fn(self.ctx, None, 0)
        self._check(min(n, 0))
        out = np.zeros((max(n, 1), 8), np.uint32)
        self._check(min(fn(self.ctx, out.ctypes.data, n), 0))
        return out[:n]

    def Resize(self, fb_width: int, fb_height: int, superSample: int):
        self._check(self.L.ycge_resize(self.ctx, fb_width, fb_height, superSample))          # (joins the frames in flight: nothing writes the old arrays any more)
        self._set_dims(fb_width, fb_height, max(1, superSample))
        self._drop_sdr_ring(keep_shape=(self.fbH, self.fbW, 2, 3))

    def _drop_sdr_ring(self, keep_shape=None):
        """The page-locked SDR arrays of the frames in flight: those of another console size go back to the library (nothing is in flight:
        the callers are Resize, which joins first, and close, after ycge_destroy)."""
        ring = self.__dict__.get("_sdr_ring", {})
        for key in [k for k, (a, _) in ring.items() if a.shape != keep_shape]:
            a, handle = ring.pop(key)
            self._free_page_locked(handle)

    def SetCamera(self, pos, yaw: float, pitch: float):
        self._pos, self._yaw, self._pitch = tuple(pos), yaw, pitch
        self._push_camera()

    def SetFov(self, fovDeg: float):
        self._fov = fovDeg
        self._push_camera()

    def _push_camera(self):
        p = (C.c_float * 3)(*self._pos)
        self._check(self.L.ycge_set_camera(self.ctx, p, self._yaw, self._pitch, self._fov))

    def _page_locked_zeros(self, shape, dtype=np.float32):
        """A zeroed float32 array in page-locked memory OF THE LIBRARY (ycge_alloc_host_buffer: hipHostMalloc): (array, owner).  The
        device writes SDR frames straight into it.  Round 4 registered numpy arrays instead (hipHostRegister) and met GPU memory faults
        at heap addresses: registration is page-granular, and - more to the point - a mapping of process heap lives and dies with the
        allocator, not with the array (csrc/ycge_host.cpp: copy_out).
        LIFETIME: the allocation belongs to the ARRAY, not to the renderer - the ctypes buffer under the numpy array carries a
        _PageLockedOwner whose finaliser hands the pages back (ycge_free_host_buffer) when the last view of the array dies.  close(),
        Resize() and a change of console size only drop the renderer's own reference (after joining the frames in flight, so the device
        is done with the pages): an array a caller still holds - TryFlipAndBlit(copy=False), RenderAsync(sdr_slot=k) - stays readable."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        rc = self.L.ycge_alloc_host_buffer(nbytes, C.byref(p))
        if rc != 0 or not p.value:
            raise abi.YcgeError(rc, f"no page-locked memory for an SDR frame of {nbytes} bytes")
        owner = _PageLockedOwner(self.L, p.value)
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        buf._ycge_owner = owner          # (numpy keeps `buf` alive through the buffer protocol; `buf` keeps the owner)
        a = np.ctypeslib.as_array(buf).view(dtype).reshape(shape)
        return a, owner

    def _free_page_locked(self, handle):
        """Drops the renderer's reference; the pages go back when no array over them is left (see _page_locked_zeros)."""
        return None

    def _sdr_buffer(self):
        """The wrapper's ONE SDR buffer (the C# side keeps one for the life of the renderer, bindings/csharp/HipRaytraceWrapper.cs), page-locked
        memory of the library: the frame's read-back is a plain DMA."""
        shape = (self.fbH, self.fbW, 2, 3)
        if getattr(self, "_sdr", None) is None or self._sdr.shape != shape:
            if getattr(self, "_sdr", None) is not None and getattr(self, "ctx", None):
                self.L.ycge_wait(self.ctx)
            self._drop_sdr_buffer()
            self._sdr, self._sdr_handle = self._page_locked_zeros(shape)
        return self._sdr

    def _drop_sdr_buffer(self):
        if getattr(self, "_sdr", None) is not None:
            self._free_page_locked(getattr(self, "_sdr_handle", None))
        self._sdr = None
        self._sdr_handle = None

    def TryFlipAndBlit(self, want_sdr: bool = False, copy: bool = True):
        """One frame.  Returns the fbH x fbW x 2 x 3 SDR array (top, bottom per chexel) when want_sdr (a copy of the wrapper's
        buffer; copy=False hands out the buffer itself: OVERWRITTEN by the next frame of this size, left alone - and valid for as long as
        the caller holds it - after Resize() to another size or close()), else the frame statistics."""
        sdr = self._sdr_buffer() if want_sdr else None
        ptr = sdr.ctypes.data_as(C.POINTER(C.c_float)) if want_sdr else None
        self._check(self.L.ycge_render_frame(self.ctx, ptr, C.byref(self.stats)))
        return (sdr.copy() if copy else sdr) if want_sdr else self.stats

    def RenderAsync(self, sdr_slot=None):
        """Frames in flight (ycge_render_frame_async): queues the next frame through TAA and returns; the trace of the frame after it
        runs beside this one's TAA.  Same frames as TryFlipAndBlit() in the same order.  Wait() - or any other call - joins.
        With sdr_slot = k the frame runs the post stage too (ycge_render_frame_async_sdr) into the wrapper's k-th page-locked SDR array,
        which is returned and holds the frame once Wait() has returned: one slot per frame in flight."""
        if sdr_slot is None:
            self._check(self.L.ycge_render_frame_async(self.ctx))
            return None
        ring = self.__dict__.setdefault("_sdr_ring", {})
        key = int(sdr_slot)
        if key in ring and ring[key][0].shape != (self.fbH, self.fbW, 2, 3):
            self._drop_sdr_ring(keep_shape=(self.fbH, self.fbW, 2, 3))
        if key not in ring:
            ring[key] = self._page_locked_zeros((self.fbH, self.fbW, 2, 3))
        a = ring[key][0]
        self._check(self.L.ycge_render_frame_async_sdr(self.ctx, a.ctypes.data_as(C.POINTER(C.c_float))))
        return a

    # ---------------------------------------------------------------- device chexel colours (ycge_render_frame_chexels)
    CHEXEL_OUTPUTS = ("sdr", "color16", "ansi", "rgba")

    def chexel_shapes(self) -> dict:
        """What each output of the chexel calls holds: sdr {top rgb, bottom rgb} f32; color16 one byte a chexel (color_16 of top | of
        bottom << 4); ansi {top, bottom} ANSI-256 indices; rgba the fbW x 2 fbH RGBA8 compose image (row 2 cy = top half-cells)."""
        return {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "color16": ((self.fbH, self.fbW), np.uint8),
                "ansi": ((self.fbH, self.fbW, 2), np.uint8), "rgba": ((2 * self.fbH, self.fbW, 4), np.uint8)}

    @staticmethod
    def _chexel_pointers(arrays: dict):
        f = arrays.get("sdr")
        u8 = lambda k: arrays[k].ctypes.data_as(C.POINTER(C.c_uint8)) if k in arrays else None
        return (f.ctypes.data_as(C.POINTER(C.c_float)) if f is not None else None), u8("color16"), u8("ansi"), u8("rgba")

    def TryFlipAndBlitChexels(self, color16: bool = True, ansi: bool = False, rgba: bool = False, sdr: bool = False) -> dict:
        """One frame (ycge_render_frame_chexels): the post stage runs whatever is asked, and the presenters' colour maps of its SDR
        array come back from the device - {name: array} for each output asked (shapes: chexel_shapes).  The SDR and the frame state are
        those of TryFlipAndBlit(want_sdr=True); the frame statistics go to self.stats."""
        want = {"sdr": sdr, "color16": color16, "ansi": ansi, "rgba": rgba}
        arrays = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in self.chexel_shapes().items() if want[k]}
        self._check(self.L.ycge_render_frame_chexels(self.ctx, *self._chexel_pointers(arrays), C.byref(self.stats)))
        return arrays

    def RenderAsyncChexels(self, slot: int, color16: bool = True, ansi: bool = False, rgba: bool = False, sdr: bool = False) -> dict:
        """Frames in flight with the chexel outputs (ycge_render_frame_async_chexels), as RenderAsync(sdr_slot=slot): the wrapper's
        page-locked arrays of this slot are returned and hold the frame once Wait() has returned - one slot per frame in flight."""
        want = {"sdr": sdr, "color16": color16, "ansi": ansi, "rgba": rgba}
        ring = self.__dict__.setdefault("_chexel_ring", {})
        arrays = {}
        for k, (shp, dt) in self.chexel_shapes().items():
            if not want[k]:
                continue
            key = (int(slot), k)
            if key not in ring or ring[key][0].shape != shp:        # (another console size: Resize joined the frames in flight)
                ring[key] = self._page_locked_zeros(shp, dt)
            arrays[k] = ring[key][0]
        self._check(self.L.ycge_render_frame_async_chexels(self.ctx, *self._chexel_pointers(arrays)))
        return arrays

    # ---------------------------------------------------------------- the ANSI escape stream (ycge_render_frame_ansi)
    @staticmethod
    def ansi_stream_bound(console_width: int, console_height: int, lib=None) -> int:
        """The most bytes the ANSI stream of a console_width x console_height console can take (ycge_ansi_stream_bound; no GPU needed)."""
        return RaytraceRenderer._ansi_bound(console_width, console_height, False, lib)

    @staticmethod
    def _ansi_bound(console_width: int, console_height: int, rgb: bool, lib=None) -> int:
        """ycge_ansi_stream_bound, or with rgb ycge_ansi_rgb_stream_bound"""
        L = lib if lib is not None else abi.load_library()
        n = C.c_size_t(0)
        rc = (L.ycge_ansi_rgb_stream_bound if rgb else L.ycge_ansi_stream_bound)(int(console_width), int(console_height), C.byref(n))
        if rc != 0:
            raise abi.YcgeError(rc, f"no {'24-bit ' if rgb else ''}ANSI stream bound for a {console_width} x {console_height} console")
        return n.value

    def _ansi_out(self, console_width: int, console_height: int, rgb: bool = False):
        """the renderer's growable page-locked stream buffer, at least the bound of this console in the colour form asked"""
        bound = self._ansi_bound(console_width, console_height, rgb, self.L)
        buf = self.__dict__.get("_ansi_buf")
        if buf is None or buf[0].size < bound:
            self.__dict__.pop("_ansi_buf", None)
            buf = self.__dict__["_ansi_buf"] = self._page_locked_zeros((bound,), np.uint8)
        return buf[0]

    def _ansi_call(self, export, head, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr, rgb=False, delta=None, stats=True, extra=()):
        """One stream call on this context: export(ctx, *head, the console, viewport, defaults and clear_screen, *delta, the stream buffer,
        its capacity and length[, info], the SDR array or NULL[, the frame statistics]).  head: a video call's frame arguments; delta: a
        _delta call's (merge_gap[, tolerance], keyframe[, min_contrast]), or None; extra: what a plain call takes behind clear_screen (the
        quadrant stream's min_contrast).  A plain call returns bytes or (bytes, SDR array), a _delta call
        (bytes, info) or (bytes, info, SDR array)."""
        out = self._ansi_out(console_width, console_height, rgb)
        n = C.c_size_t(0)
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        console = (int(console_width), int(console_height), int(viewport[0]), int(viewport[1]), int(default_fg), int(default_bg), int(bool(clear_screen)))
        buf = (out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, C.byref(n))
        tail = (s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None,) + ((C.byref(self.stats),) if stats else ())
        if delta is None:
            self._check(export(self.ctx, *head, *console, *(int(v) for v in extra), *buf, *tail))
            stream = out[:n.value].tobytes()
            return (stream, s) if sdr else stream
        info = (C.c_uint32 * 4)()
        self._check(export(self.ctx, *head, *console, *(int(v) for v in delta), *buf, info, *tail))
        stream, info = out[:n.value].tobytes(), dict(zip(self.DELTA_INFO, (int(v) for v in info)))
        return (stream, info, s) if sdr else (stream, info)

    def TryFlipAndBlitAnsi(self, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                           clear_screen: bool = False, sdr: bool = False):
        """One frame (ycge_render_frame_ansi): the bytes ANSITerminalRenderer.Render() writes for a console over this framebuffer at
        `viewport`, built on the device - `bytes`, or (bytes, SDR array) with sdr=True.  The SDR and the frame state are those of
        TryFlipAndBlit(want_sdr=True); the frame statistics go to self.stats.  The stream is read back into one growable page-locked
        buffer of the renderer, freed by close()."""
        return self._ansi_call(self.L.ycge_render_frame_ansi, (), console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr)

    DELTA_INFO = ("keyframe", "changed", "emitted", "runs")

    def TryFlipAndBlitAnsiDelta(self, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                                clear_screen: bool = False, merge_gap: int = 3, keyframe: bool = False, sdr: bool = False):
        """One frame (ycge_render_frame_ansi_delta): the bytes that bring a terminal showing this context's last stream to this frame -
        only the cells that changed, or the whole stream of TryFlipAndBlitAnsi when a keyframe is due (the first call, another
        geometry, clear_screen, keyframe, after Resize or a plain TryFlipAndBlitAnsi).  Returns (bytes, info) or (bytes, info, SDR
        array) with sdr=True; info = {"keyframe", "changed", "emitted", "runs"}.  The frame state is TryFlipAndBlit's."""
        return self._ansi_call(self.L.ycge_render_frame_ansi_delta, (), console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr,
                               delta=(merge_gap, bool(keyframe)))

    # ---------------------------------------------------------------- the 24-bit colour forms (ycge_render_frame_ansi_rgb / _rgb_delta)
    @staticmethod
    def ansi_rgb_stream_bound(console_width: int, console_height: int, lib=None) -> int:
        """The most bytes a 24-bit colour stream of a console_width x console_height console can take (ycge_ansi_rgb_stream_bound; no GPU needed)."""
        return RaytraceRenderer._ansi_bound(console_width, console_height, True, lib)

    def TryFlipAndBlitAnsiRgb(self, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                              clear_screen: bool = False, sdr: bool = False):
        """TryFlipAndBlitAnsi in 24-bit colour (ycge_render_frame_ansi_rgb): the same walk with ESC[38;2;R;G;Bm / ESC[48;2;R;G;Bm of the
        sRGB8 triples TryFlipAndBlit(rgba=True) gives - `bytes`, or (bytes, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_render_frame_ansi_rgb, (), console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr, rgb=True)

    def TryFlipAndBlitAnsiRgbDelta(self, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                                   clear_screen: bool = False, merge_gap: int = 3, tolerance: int = 0, keyframe: bool = False, sdr: bool = False):
        """TryFlipAndBlitAnsiDelta in 24-bit colour (ycge_render_frame_ansi_rgb_delta): a cell is rewritten when a channel is more than
        `tolerance` (0..255; 0 = exact) away from what the terminal shows for it.  One terminal per context: a stream of the other colour
        form makes the next call a keyframe.  Returns (bytes, info) or (bytes, info, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_render_frame_ansi_rgb_delta, (), console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr,
                               rgb=True, delta=(merge_gap, tolerance, bool(keyframe)))

    # ---------------------------------------------------------------- quadrant-glyph frames (ycge_render_frame_quadrants / _ansi_quad / _ansi_quad_delta)
    QUADRANT_GLYPHS = (0x2580, 0x2598, 0x259D, 0x2580, 0x2596, 0x258C, 0x259E, 0x259B)      # by mask: bit 0 = TL, bit 1 = TR, bit 2 = BL in the foreground

    def TryFlipAndBlitQuadrants(self, quad_sdr: bool = False, glyphs: bool = True, rgba: bool = True, sdr: bool = False, min_contrast: int = 0) -> dict:
        """One frame (ycge_render_frame_quadrants; super_sample must be even): each chexel's 2 x 2 sub-cell colours and the quadrant block
        glyph and two colours fitted to them on the device - {name: array} for each output asked: "quad_sdr" (fbH, fbW, 4, 3) f32 {TL, TR,
        BL, BR}; "glyphs" (fbH, fbW) uint16 code units; "rgba" (2 fbH, fbW, 4) uint8, row 2 cy the foreground and row 2 cy + 1 the
        background; "sdr" as TryFlipAndBlitChexels.  min_contrast (0..255): a chexel whose sub-cell bytes all lie within it of their mean
        stays one colour.  The SDR and the frame state are those of TryFlipAndBlit(want_sdr=True); the statistics go to self.stats."""
        shapes = {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "quad_sdr": ((self.fbH, self.fbW, 4, 3), np.float32),
                  "glyphs": ((self.fbH, self.fbW), np.uint16), "rgba": ((2 * self.fbH, self.fbW, 4), np.uint8)}
        want = {"sdr": sdr, "quad_sdr": quad_sdr, "glyphs": glyphs, "rgba": rgba}
        arrays = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if want[k]}
        ptr = lambda k, t: arrays[k].ctypes.data_as(C.POINTER(t)) if k in arrays else None
        self._check(self.L.ycge_render_frame_quadrants(self.ctx, ptr("sdr", C.c_float), ptr("quad_sdr", C.c_float), ptr("glyphs", C.c_uint16), ptr("rgba", C.c_uint8),
                                                       int(min_contrast), C.byref(self.stats)))
        return arrays

    def TryFlipAndBlitAnsiQuad(self, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                               clear_screen: bool = False, min_contrast: int = 0, sdr: bool = False):
        """TryFlipAndBlitAnsiRgb with quadrant block glyphs (ycge_render_frame_ansi_quad): a covered cell's character and triples are the
        glyph, foreground and background TryFlipAndBlitQuadrants gives - `bytes`, or (bytes, SDR array) with sdr=True.  The bound is
        ansi_rgb_stream_bound; super_sample must be even."""
        return self._ansi_call(self.L.ycge_render_frame_ansi_quad, (), console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr, rgb=True,
                               extra=(min_contrast,))

    def TryFlipAndBlitAnsiQuadDelta(self, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                                    clear_screen: bool = False, merge_gap: int = 3, tolerance: int = 0, keyframe: bool = False, min_contrast: int = 0,
                                    sdr: bool = False):
        """TryFlipAndBlitAnsiRgbDelta with quadrant block glyphs (ycge_render_frame_ansi_quad_delta): a cell is rewritten when its glyph
        differs from what the terminal shows or a channel is more than `tolerance` away.  A third family beside the 256-colour and 24-bit
        streams: a stream of another family makes the next call a keyframe.  Returns (bytes, info) or (bytes, info, SDR array)."""
        return self._ansi_call(self.L.ycge_render_frame_ansi_quad_delta, (), console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr,
                               rgb=True, delta=(merge_gap, tolerance, bool(keyframe), min_contrast))

    # ---------------------------------------------------------------- sixel frames (ycge_render_frame_pixels / _sixel)
    @staticmethod
    def sixel_stream_bound(px_width: int, px_height: int, lib=None) -> int:
        """The most bytes the sixel stream of a px_width x px_height picture can take (ycge_sixel_stream_bound; no GPU needed)."""
        L = lib if lib is not None else abi.load_library()
        n = C.c_size_t(0)
        rc = L.ycge_sixel_stream_bound(int(px_width), int(px_height), C.byref(n))
        if rc != 0:
            raise abi.YcgeError(rc, f"no sixel stream bound for a {px_width} x {px_height} picture")
        return n.value

    def TryFlipAndBlitPixels(self, rgba: bool = True, index: bool = True, dither: bool = False, sdr: bool = False) -> dict:
        """One frame (ycge_render_frame_pixels): every hi-res sample the frame traced as a pixel - {name: array} for each output asked:
        "rgba" (2 fbH ss, fbW ss, 4) uint8, the sRGB8 bytes with alpha 255; "index" (2 fbH ss, fbW ss) uint8, its register in the
        6 x 6 x 6 cube of the sixel stream (ordered 4 x 4 dither on request); "sdr" as TryFlipAndBlitChexels.  The SDR and the frame
        state are those of TryFlipAndBlit(want_sdr=True); the statistics go to self.stats.  The ANSI delta state is left alone."""
        W, H = self.fbW * self.ss, 2 * self.fbH * self.ss
        shapes = {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "rgba": ((H, W, 4), np.uint8), "index": ((H, W), np.uint8)}
        want = {"sdr": sdr, "rgba": rgba, "index": index}
        arrays = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if want[k]}
        ptr = lambda k, t: arrays[k].ctypes.data_as(C.POINTER(t)) if k in arrays else None
        self._check(self.L.ycge_render_frame_pixels(self.ctx, ptr("sdr", C.c_float), ptr("rgba", C.c_uint8), ptr("index", C.c_uint8), int(bool(dither)),
                                                    C.byref(self.stats)))
        return arrays

    def TryFlipAndBlitSixel(self, viewport=(0, 0), clear_screen: bool = False, dither: bool = False, sdr: bool = False):
        """One frame (ycge_render_frame_sixel): the DEC sixel stream of TryFlipAndBlitPixels' registers with its top left corner at cell
        `viewport`, built on the device - `bytes`, or (bytes, SDR array) with sdr=True.  The picture paints over the terminal's cells: the
        next _delta call of any family returns a keyframe.  The stream is read back into one growable pageable buffer of the renderer of
        the bound's size, of which only the pages a stream reaches are ever backed."""
        bound = self.sixel_stream_bound(self.fbW * self.ss, 2 * self.fbH * self.ss, self.L)
        buf = self.__dict__.get("_sixel_buf")
        if buf is None or buf.size < bound:
            buf = self.__dict__["_sixel_buf"] = np.empty(bound, np.uint8)
        n = C.c_size_t(0)
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        self._check(self.L.ycge_render_frame_sixel(self.ctx, int(viewport[0]), int(viewport[1]), int(bool(clear_screen)), int(bool(dither)),
                                                   buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(n),
                                                   s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None, C.byref(self.stats)))
        stream = buf[:n.value].tobytes()
        return (stream, s) if sdr else stream

    def _sixel_buffer(self):
        bound = self.sixel_stream_bound(self.fbW * self.ss, 2 * self.fbH * self.ss, self.L)
        buf = self.__dict__.get("_sixel_buf")
        if buf is None or buf.size < bound:
            buf = self.__dict__["_sixel_buf"] = np.empty(bound, np.uint8)
        return buf

    def TryFlipAndBlitSixelDelta(self, viewport=(0, 0), clear_screen: bool = False, keyframe: bool = False, dither: bool = False, sdr: bool = False):
        """One frame (ycge_render_frame_sixel_delta): the sixel stream that repaints only the bands and columns whose registers differ from
        the last sixel stream this context handed out - or TryFlipAndBlitSixel's bytes, a keyframe, when there is no such stream, the
        geometry or viewport changed, or clear_screen / keyframe ask for one.  (bytes, info) or (bytes, info, SDR array) with sdr=True;
        info = (keyframe returned, changed bands, pixels painted, lines).  The state is the one the ANSI _delta calls and
        VideoRenderer.TryFlipAndBlitSixelDelta share."""
        buf, n, info = self._sixel_buffer(), C.c_size_t(0), (C.c_uint32 * 4)()
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        self._check(self.L.ycge_render_frame_sixel_delta(self.ctx, int(viewport[0]), int(viewport[1]), int(bool(clear_screen)), int(bool(keyframe)), int(bool(dither)),
                                                         buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(n), info,
                                                         s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None, C.byref(self.stats)))
        stream = buf[:n.value].tobytes()
        return (stream, tuple(info), s) if sdr else (stream, tuple(info))

    # ---------------------------------------------------------------- the adaptive sixel palette (ycge_render_frame_sixel_palette / _pixels_palette)
    @staticmethod
    def sixel_palette_stream_bound(px_width: int, px_height: int, lib=None) -> int:
        """The most bytes the adaptive-palette sixel stream of a px_width x px_height picture can take (ycge_sixel_palette_stream_bound; no GPU needed)."""
        L = lib if lib is not None else abi.load_library()
        n = C.c_size_t(0)
        rc = L.ycge_sixel_palette_stream_bound(int(px_width), int(px_height), C.byref(n))
        if rc != 0:
            raise abi.YcgeError(rc, f"no sixel stream bound for a {px_width} x {px_height} picture")
        return n.value

    def _sixel_palette_buffer(self):
        bound = self.sixel_palette_stream_bound(self.fbW * self.ss, 2 * self.fbH * self.ss, self.L)
        buf = self.__dict__.get("_sixel_buf")
        if buf is None or buf.size < bound:
            buf = self.__dict__["_sixel_buf"] = np.empty(bound, np.uint8)
        return buf

    def TryFlipAndBlitSixelPalette(self, viewport=(0, 0), clear_screen: bool = False, hold: bool = False, sdr: bool = False):
        """One frame (ycge_render_frame_sixel_palette): the sixel stream of the frame's pixels under an adaptive palette - up to 256
        median-cut registers built on the device from this picture, or with hold=True the palette the context kept from the last build
        (none kept: built).  (bytes, palette (256, 4) uint8 - the registers' bytes, alpha 255, unused entries zero -, count), and the SDR
        array behind them with sdr=True.  The next _delta call of any family returns a keyframe."""
        buf, n = self._sixel_palette_buffer(), C.c_size_t(0)
        palette, count = np.zeros((256, 4), np.uint8), C.c_int32(0)
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        self._check(self.L.ycge_render_frame_sixel_palette(self.ctx, int(viewport[0]), int(viewport[1]), int(bool(clear_screen)), int(bool(hold)),
                                                           buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(n), palette.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                           C.byref(count), s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None, C.byref(self.stats)))
        stream = buf[:n.value].tobytes()
        return (stream, palette, count.value, s) if sdr else (stream, palette, count.value)

    def TryFlipAndBlitPixelsPalette(self, rgba: bool = True, index: bool = True, hold: bool = False, sdr: bool = False) -> dict:
        """One frame (ycge_render_frame_pixels_palette): TryFlipAndBlitPixels' planes with the adaptive palette's registers in "index", and
        "palette" (256, 4) uint8 and "count" with them.  The delta state is left alone; the palette is kept as TryFlipAndBlitSixelPalette keeps it."""
        W, H = self.fbW * self.ss, 2 * self.fbH * self.ss
        shapes = {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "rgba": ((H, W, 4), np.uint8), "index": ((H, W), np.uint8), "palette": ((256, 4), np.uint8)}
        want = {"sdr": sdr, "rgba": rgba, "index": index, "palette": True}
        arrays = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if want[k]}
        ptr = lambda k, t: arrays[k].ctypes.data_as(C.POINTER(t)) if k in arrays else None
        count = C.c_int32(0)
        self._check(self.L.ycge_render_frame_pixels_palette(self.ctx, ptr("sdr", C.c_float), ptr("rgba", C.c_uint8), ptr("index", C.c_uint8), int(bool(hold)),
                                                            ptr("palette", C.c_uint8), C.byref(count), C.byref(self.stats)))
        arrays["count"] = count.value
        return arrays

    # ---------------------------------------------------------------- ANSI streams with frames in flight (ycge_render_frame_async_ansi)
    def RenderAsyncAnsi(self, slot: int, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                        clear_screen: bool = False, rgb: bool = False, delta: bool = False, merge_gap: int = 3, tolerance: int = 0,
                        keyframe: bool = False, sdr: bool = False) -> None:
        """Frames in flight with the ANSI stream (ycge_render_frame_async_ansi), as RenderAsyncChexels: queues the frame and returns.  The
        four forms of TryFlipAndBlitAnsi / AnsiDelta / AnsiRgb / AnsiRgbDelta by `rgb` and `delta`; merge_gap and keyframe are read with
        delta alone, tolerance with rgb and delta.  The stream is delivered on the device into the wrapper's page-locked buffer of this
        slot - one slot per frame in flight - and AsyncAnsiResult(slot) hands it out once Wait() has returned.  The bytes are those the
        synchronous call of the same form would have returned in its place; a queued delta counts as handed out when it is queued."""
        bound = self._ansi_bound(console_width, console_height, rgb, self.L)
        ring = self.__dict__.setdefault("_ansi_ring", {})
        key = int(slot)
        if key not in ring or ring[key]["stream"].size < bound:            # (the first frame of a larger console: nothing of this slot may be in flight)
            if key in ring:
                self.Wait()
            ring[key] = {"stream": self._page_locked_zeros((bound,), np.uint8)[0], "record": self._page_locked_zeros((C.sizeof(abi.AnsiAsyncResult),), np.uint8)[0]}
        entry = ring[key]
        shape = (self.fbH, self.fbW, 2, 3)
        if sdr and (entry.get("sdr") is None or entry["sdr"].shape != shape):
            entry["sdr"] = self._page_locked_zeros(shape)[0]
        entry["want_sdr"] = bool(sdr)
        req = abi.AnsiAsync(int(console_width), int(console_height), int(viewport[0]), int(viewport[1]), int(default_fg), int(default_bg), int(bool(clear_screen)),
                            int(bool(rgb)), int(bool(delta)), int(merge_gap) if delta else 0, int(tolerance) if (delta and rgb) else 0, int(bool(keyframe)) if delta else 0)
        out = entry["stream"]
        self._check(self.L.ycge_render_frame_async_ansi(self.ctx, C.byref(req), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size, entry["record"].ctypes.data,
                                                        entry["sdr"].ctypes.data_as(C.POINTER(C.c_float)) if sdr else None))

    def AsyncAnsiResult(self, slot: int):
        """What the frame queued last into `slot` delivered - valid after Wait(): (bytes, info) or, when it was queued with sdr=True,
        (bytes, info, SDR array), info as TryFlipAndBlitAnsiDelta's (a full stream: keyframe 1, the counts 0).  Raises when the record's
        status is not 0 (the device stream exceeded the buffer; nothing was copied)."""
        entry = self.__dict__.get("_ansi_ring", {})[int(slot)]
        rec = abi.AnsiAsyncResult.from_buffer_copy(entry["record"].tobytes())
        if rec.status != 0:
            raise abi.YcgeError(abi.YCGE_ERR_DEVICE, f"the ANSI stream of slot {slot} was not delivered (status {rec.status}, length {rec.length})")
        stream, info = entry["stream"][:rec.length].tobytes(), dict(zip(self.DELTA_INFO, (int(v) for v in rec.info)))
        return (stream, info, entry["sdr"]) if entry["want_sdr"] else (stream, info)

    # ---------------------------------------------------------------- the console's other framebuffers (ycge_console_set_layers)
    def SetConsoleLayers(self, layers=(), raytrace_at: int = 0):
        """The console's OTHER framebuffers for every TryFlipAndBlitAnsi* call of this context from now on (ycge_console_set_layers): a
        sequence of ConsoleLayer in frameBuffers order, bottom first, of which `raytrace_at` lie below the raytrace framebuffer.  The
        streams are then Render()'s for the whole list - GetChexelForPoint over every framebuffer, any character.  An empty sequence
        removes the layers.  The cells are copied; a refused call (abi.YcgeError) leaves the previous layers in force."""
        layers = list(layers)
        arr = (abi.ConsoleLayer * max(1, len(layers)))()
        for k, l in enumerate(layers):
            arr[k] = l.as_struct()
        self._check(self.L.ycge_console_set_layers(self.ctx, arr if layers else None, len(layers), int(raytrace_at)))

    def Wait(self):
        self._check(self.L.ycge_wait(self.ctx))

    def flight_info(self) -> dict:
        """What the frames-in-flight machinery of this context does (ycge_flight_query): timing only, never a pixel."""
        fi = abi.FlightInfo()
        self._check(self.L.ycge_flight_query(self.ctx, C.byref(fi)))
        return {f: int(getattr(fi, f)) for f, _ in abi.FlightInfo._fields_}

    def async_trace_ms(self, capacity: int = 1024) -> np.ndarray:
        """Durations (ms) of the trace launches of the frames queued since the last call (waits for them), oldest first."""
        a = np.zeros(capacity, dtype=np.float32)
        n = C.c_int32()
        self._check(self.L.ycge_async_trace_times(self.ctx, a.ctypes.data_as(C.POINTER(C.c_float)), capacity, C.byref(n)))
        return a[:n.value].copy()

    # ---------------------------------------------------------------- multi-GPU halves
    def tile_slab_bytes(self) -> int:
        n = C.c_size_t()
        self._check(self.L.ycge_tile_slab_bytes(self.ctx, C.byref(n)))
        return n.value

    def trace_tiles(self, d_slab_ptr: int, stream_ptr: int = 0, want_stats: bool = False):
        st = C.byref(self.stats) if want_stats else None
        self._check(self.L.ycge_trace_tiles(self.ctx, C.c_void_p(d_slab_ptr), C.c_void_p(stream_ptr), st))

    def resolve_gathered(self, d_all_slabs_ptr: int, stream_ptr: int = 0, want_stats: bool = False, want_sdr: bool = False):
        """TAA on the gathered frame; with want_sdr also the denoise / exposure / tonemap stage (needs slab_albedo), returns the SDR array."""
        st = C.byref(self.stats) if want_stats else None
        sdr = np.zeros((self.fbH, self.fbW, 2, 3), dtype=np.float32) if want_sdr else None
        ptr = sdr.ctypes.data_as(C.POINTER(C.c_float)) if want_sdr else None
        self._check(self.L.ycge_resolve_gathered(self.ctx, C.c_void_p(d_all_slabs_ptr), C.c_void_p(stream_ptr), ptr, st))
        return sdr

    # the tile-resident form (include/ycge.h): TAA on this rank's own tiles, a halo exchange instead of the all-gather of slabs
    def halo_counts(self):
        w = self.cfg.world_size
        s, r = (C.c_int64 * w)(), (C.c_int64 * w)()
        self._check(self.L.ycge_halo_counts(self.ctx, s, r))
        return list(s), list(r)

    def history_slab_bytes(self) -> int:
        n = C.c_size_t()
        self._check(self.L.ycge_history_slab_bytes(self.ctx, C.byref(n)))
        return n.value

    def trace_tiles_resident(self, d_halo_send_ptr: int, stream_ptr: int = 0, want_stats: bool = False):
        st = C.byref(self.stats) if want_stats else None
        self._check(self.L.ycge_trace_tiles_resident(self.ctx, C.c_void_p(d_halo_send_ptr), C.c_void_p(stream_ptr), st))

    def trace_tiles_resident_batch(self, poses, d_halo_send_ptrs, stream_ptr: int = 0):
        """n consecutive frames of this rank's tiles in one launch (ycge_trace_tiles_resident_batch): poses = n x (pos, yaw, pitch, fov)."""
        n = len(poses)
        flat = (C.c_float * (6 * n))()
        for k, (pos, yaw, pitch, fov) in enumerate(poses):
            flat[6 * k:6 * k + 6] = [pos[0], pos[1], pos[2], yaw, pitch, fov]
        ptrs = (C.c_void_p * n)(*[C.c_void_p(p) for p in d_halo_send_ptrs])
        self._check(self.L.ycge_trace_tiles_resident_batch(self.ctx, n, flat, ptrs, C.c_void_p(stream_ptr)))

    def resolve_tiles_resident(self, d_halo_recv_ptr: int, d_history_slab_ptr: int = 0, stream_ptr: int = 0, want_stats: bool = False):
        st = C.byref(self.stats) if want_stats else None
        self._check(self.L.ycge_resolve_tiles_resident(self.ctx, C.c_void_p(d_halo_recv_ptr), C.c_void_p(d_history_slab_ptr), C.c_void_p(stream_ptr), st))

    def unpack_history(self, d_all_history_slabs_ptr: int, stream_ptr: int = 0):
        self._check(self.L.ycge_unpack_history(self.ctx, C.c_void_p(d_all_history_slabs_ptr), C.c_void_p(stream_ptr)))

    # ---------------------------------------------------------------- tests only
    def set_frame_counter(self, n: int):
        self._check(self.L.ycge_set_frame_counter(self.ctx, n))

    def timed_steps(self) -> int:
        """Cumulative traversal-loop steps (summed over lanes, all devices) of the timed kernel instances (ycge_read_timed_steps)."""
        n = C.c_uint64()
        self._check(self.L.ycge_read_timed_steps(self.ctx, C.byref(n)))
        return int(n.value)

    def _post_hook(self, name: str):
        fn = getattr(self.L, name)
        fn.restype, fn.argtypes = abi.POST_HOOK_PROTOTYPES[name]
        return fn

    @staticmethod
    def _post_state(words: np.ndarray) -> dict:
        f = words.view(np.float32)
        return dict(ae_exposure=f[0], effective=f[1], serial_chunks=int(words[2]), log_sum=f[4], count=int(words[5]))

    def post_probe(self, hist, albedo, normal, depth, sky, ae_in: float = 1.0):
        """Steps 6-8 of TryFlipAndBlit on caller-given hiH x hiW arrays (ycge_test_post_stage): the frames' own post stage, with this
        renderer's config and knobs.  Returns (denoised, sdr, state) with state = {ae_exposure, effective, serial_chunks, log_sum, count}.
        Overwrites the TAA history, the G-buffer and the exposure state of the context."""
        n = self.hiH * self.hiW
        arrs = []
        for a, dt, k in ((hist, np.float32, 3 * n), (albedo, np.float32, 3 * n), (normal, np.float32, 3 * n), (depth, np.float32, n), (sky, np.uint8, n)):
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != k:
                raise ValueError(f"post_probe: an array of {a.size} elements where the {self.hiW} x {self.hiH} trace grid needs {k}")
            arrs.append(a)
        den = np.zeros((self.hiH, self.hiW, 3), np.float32)
        sdr = np.zeros((self.fbH, self.fbW, 2, 3), np.float32)
        st = np.zeros(abi.POST_STATE_WORDS, np.uint32)
        self._check(self._post_hook("ycge_test_post_stage")(self.ctx, *[a.ctypes.data for a in arrs], float(ae_in), den.ctypes.data, sdr.ctypes.data, st.ctypes.data))
        return den, sdr, self._post_state(st)

    def exposure_probe(self, terms, ae_in: float = 1.0, serial: bool = False) -> dict:
        """The exposure sum kernels alone (ycge_test_exposure) on a vector of log terms, 0 = a skipped sample; the state as post_probe's."""
        t = np.ascontiguousarray(terms, dtype=np.float32).ravel()
        st = np.zeros(abi.POST_STATE_WORDS, np.uint32)
        self._check(self._post_hook("ycge_test_exposure")(self.ctx, t.ctypes.data, t.size, float(ae_in), int(bool(serial)), st.ctypes.data))
        return self._post_state(st)

    def taa_probe(self, form: int, reset: bool, current, normal, depth, sky, hist_in, prev_normal, prev_depth, prev_sky,
                  taa_alpha: float = 0.01, taa_clamp_radius: int = 1, taa_luminance_pad: float = 0.10) -> dict:
        """TemporalBlendWithClamp's kernels alone (ycge_test_taa) on caller-given h x w planes, the size read off `depth`; form: abi.TAA_FORM_*.
        The three last arguments are the raw config values.  Returns dict(hist, prev_normal, prev_depth, prev_sky) after the launch and, for
        the tile forms (which run at this context's own trace grid, as its rank of world_size), slab.  Works in buffers of its own; the tile forms create the context's tile-resident ring if it has none."""
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        if depth.ndim != 2:
            raise ValueError("taa_probe: depth is an h x w plane")
        h, w = depth.shape
        n = h * w
        arrs = [None] * 8
        for k, (a, dt, per) in enumerate(((current, np.float32, 3), (normal, np.float32, 3), (depth, np.float32, 1), (sky, np.uint8, 1), (hist_in, np.float32, 3),
                                          (prev_normal, np.float32, 3), (prev_depth, np.float32, 1), (prev_sky, np.uint8, 1))):
            a = np.ascontiguousarray(a, dtype=dt)
            if a.size != per * n:
                raise ValueError(f"taa_probe: an array of {a.size} elements where the {w} x {h} planes need {per * n}")
            arrs[k] = a
        out = dict(hist=np.zeros((h, w, 3), np.float32), prev_normal=np.zeros((h, w, 3), np.float32), prev_depth=np.zeros((h, w), np.float32),
                   prev_sky=np.zeros((h, w), np.uint8))
        slab = np.zeros(self.history_slab_bytes() // 4, np.float32) if form >= abi.TAA_FORM_SCATTER_TILES else None
        fn = self.L.ycge_test_taa
        fn.restype, fn.argtypes = abi.TAA_HOOK_PROTOTYPES["ycge_test_taa"]
        self._check(fn(self.ctx, int(form), int(bool(reset)), w, h, *[a.ctypes.data for a in arrs], float(taa_alpha), int(taa_clamp_radius), float(taa_luminance_pad),
                       out["hist"].ctypes.data, out["prev_normal"].ctypes.data, out["prev_depth"].ctypes.data, out["prev_sky"].ctypes.data,
                       slab.ctypes.data if slab is not None else None))
        if slab is not None:
            out["slab"] = slab
        return out

    def read(self, which: int) -> np.ndarray:
        dt, n = abi.BUFFER_LAYOUT[which]
        shape = (self.hiH, self.hiW, n) if n > 1 else (self.hiH, self.hiW)
        a = np.zeros(shape, dtype=dt)
        self._check(self.L.ycge_read_buffer(self.ctx, which, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return a

    def accel(self, which: int, index: int = 0) -> np.ndarray:
        n = C.c_size_t()
        self._check(self.L.ycge_accel_size(self.ctx, which, index, C.byref(n)))
        dt = NODE_DTYPE if which in (abi.ACCEL_SCENE_NODES, abi.ACCEL_MESH_NODES) else np.dtype("<i4")
        a = np.zeros(n.value // dt.itemsize, dtype=dt)
        if n.value:
            self._check(self.L.ycge_read_accel(self.ctx, which, index, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return a

    def device_info(self):
        name = C.create_string_buffer(256)
        cu = C.c_int32()
        self._check(self.L.ycge_device_info(self.ctx, name, 256, C.byref(cu)))
        return name.value.decode(), cu.value


def video_tables(src_width: int, src_height: int, fb_width: int, fb_height: int, superSample: int = 1, lib=None):
    """The tables k_video_blit reads for a src_width x src_height frame on a fb_width x fb_height console (ycge_host_video_tables; host
    only, no GPU needed): (x0 int32[hiW], wx f32[hiW, 6], y0 int32[hiH], wy f32[hiH, 6], (scale, offX, offY))."""
    L = lib if lib is not None else abi.load_library()
    fn = L.ycge_host_video_tables
    fn.restype, fn.argtypes = abi.VIDEO_HOOK_PROTOTYPES["ycge_host_video_tables"]
    ss = max(1, int(superSample))
    hiW, hiH = fb_width * ss, fb_height * 2 * ss
    x0, wx = np.zeros(hiW, np.int32), np.zeros((hiW, 6), np.float32)
    y0, wy = np.zeros(hiH, np.int32), np.zeros((hiH, 6), np.float32)
    geom = np.zeros(3, np.float32)
    rc = fn(int(src_width), int(src_height), int(fb_width), int(fb_height), ss, x0.ctypes.data, wx.ctypes.data, y0.ctypes.data, wy.ctypes.data, geom.ctypes.data)
    if rc != 0:
        raise abi.YcgeError(rc, (L.ycge_last_error(None) or b"").decode())
    return x0, wx, y0, wy, tuple(geom)


class VideoRenderer:
    """Host-side mirror of the reference's other renderer behind the IConsoleRenderer seam (Renderer/VideoRenderer.cs; VideoWrapper,
    RaytraceEntity.cs:38-50): TryFlipAndBlit resamples the frame a reader shows (Lanczos-3, letterboxed) into the console's chexels, on the
    device (ycge_video_blit).  Built over a RaytraceRenderer's context - the mode switch of RaytraceEntity: both renderers of one console -
    or over a context of its own, which needs no scene.  The readers (ffmpeg, camera) stay on the host: a frame is a numpy uint8 array of
    shape (height, width, 3) BGR or (height, width, 4) BGRA, what IFrameReader.GetCurrentFramePtr() points at."""

    def __init__(self, fb_width: int = 0, fb_height: int = 0, superSample: int = 1, *, renderer: Optional[RaytraceRenderer] = None, lib=None, device: int = 0):
        self._own = renderer is None
        self._r = renderer if renderer is not None else RaytraceRenderer(None, fb_width, fb_height, superSample=superSample, lib=lib, device=device)
        self.L = self._r.L

    fbW = property(lambda self: self._r.fbW)
    fbH = property(lambda self: self._r.fbH)
    ss = property(lambda self: self._r.ss)
    ctx = property(lambda self: self._r.ctx)

    def close(self):
        if self._own:
            self._r.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def SetCamera(self, pos, yaw: float, pitch: float):          # VideoWrapper.SetCamera / SetFov: no-ops (RaytraceEntity.cs:44-45)
        return None

    def SetFov(self, fovDeg: float):
        return None

    def Resize(self, fb_width: int, fb_height: int, superSample: int):
        """VideoWrapper.Resize makes a new VideoRenderer for the new console: the context's geometry follows (ycge_resize)."""
        self._r.Resize(fb_width, fb_height, superSample)

    @staticmethod
    def _frame_args(frame):
        f = np.asarray(frame)
        if f.dtype != np.uint8 or f.ndim != 3 or not f.flags.c_contiguous:
            raise ValueError("a video frame is a C-contiguous uint8 array of shape (height, width, 3 or 4)")
        return f, f.ctypes.data_as(C.POINTER(C.c_uint8)), int(f.shape[1]), int(f.shape[0]), int(f.shape[2])

    def TryFlipAndBlit(self, frame, color16: bool = True, ansi: bool = False, rgba: bool = False, sdr: bool = False, out: Optional[dict] = None) -> dict:
        """VideoRenderer.TryFlipAndBlit for `frame`: {name: array} for each output asked (shapes: RaytraceRenderer.chexel_shapes) - the SDR
        {topAvg, botAvg} of VideoRenderer.cs:127-128 bit for bit, and the presenters' colour maps of it.  `out` = caller's arrays to fill
        instead (any of sdr / color16 / ansi / rgba; pageable or page-locked)."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        if out is None:
            want = {"sdr": sdr, "color16": color16, "ansi": ansi, "rgba": rgba}
            out = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in self._r.chexel_shapes().items() if want[k]}
        self._r._check(self.L.ycge_video_blit(self.ctx, ptr, w, h, bpp, *RaytraceRenderer._chexel_pointers(out)))
        return out

    def SetConsoleLayers(self, layers=(), raytrace_at: int = 0):
        """RaytraceRenderer.SetConsoleLayers on the shared context: one console, whichever renderer shows on it"""
        self._r.SetConsoleLayers(layers, raytrace_at)

    def _ansi_call(self, export, frame, *args, **kwargs):
        """RaytraceRenderer._ansi_call on this context with `frame` ahead of the console: a video call carries no frame statistics"""
        f, ptr, w, h, bpp = self._frame_args(frame)
        return self._r._ansi_call(export, (ptr, w, h, bpp), *args, stats=False, **kwargs)

    def TryFlipAndBlitAnsi(self, frame, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                           clear_screen: bool = False, sdr: bool = False):
        """The bytes ANSITerminalRenderer.Render() writes for a console over this framebuffer showing `frame` (ycge_video_blit_ansi):
        `bytes`, or (bytes, SDR array) with sdr=True.  The stream buffer is the RaytraceRenderer's (page-locked, growable)."""
        return self._ansi_call(self.L.ycge_video_blit_ansi, frame, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr)

    def TryFlipAndBlitAnsiDelta(self, frame, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                                clear_screen: bool = False, merge_gap: int = 3, keyframe: bool = False, sdr: bool = False):
        """The delta form of TryFlipAndBlitAnsi (ycge_video_blit_ansi_delta), on the delta state this context shares with
        RaytraceRenderer.TryFlipAndBlitAnsiDelta: (bytes, info) or (bytes, info, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_video_blit_ansi_delta, frame, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr,
                               delta=(merge_gap, bool(keyframe)))

    def TryFlipAndBlitAnsiRgb(self, frame, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                              clear_screen: bool = False, sdr: bool = False):
        """TryFlipAndBlitAnsi in 24-bit colour (ycge_video_blit_ansi_rgb): `bytes`, or (bytes, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_video_blit_ansi_rgb, frame, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr, rgb=True)

    def TryFlipAndBlitAnsiRgbDelta(self, frame, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                                   clear_screen: bool = False, merge_gap: int = 3, tolerance: int = 0, keyframe: bool = False, sdr: bool = False):
        """The delta form of TryFlipAndBlitAnsiRgb (ycge_video_blit_ansi_rgb_delta), on the delta state this context shares with
        RaytraceRenderer.TryFlipAndBlitAnsiRgbDelta: (bytes, info) or (bytes, info, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_video_blit_ansi_rgb_delta, frame, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr,
                               rgb=True, delta=(merge_gap, tolerance, bool(keyframe)))

    # ---------------------------------------------------------------- quadrant glyphs (ycge_video_blit_quadrants / _ansi_quad / _ansi_quad_delta)
    def TryFlipAndBlitQuadrants(self, frame, quad_sdr: bool = False, glyphs: bool = True, rgba: bool = True, sdr: bool = False, min_contrast: int = 0,
                                out: Optional[dict] = None) -> dict:
        """RaytraceRenderer.TryFlipAndBlitQuadrants for `frame` (ycge_video_blit_quadrants; super_sample must be even): {name: array} for
        each output asked - "quad_sdr" (fbH, fbW, 4, 3) f32 {TL, TR, BL, BR}, each the saturated average of its ss / 2 x ss Lanczos samples;
        "glyphs" (fbH, fbW) uint16; "rgba" (2 fbH, fbW, 4) uint8, row 2 cy the foreground; "sdr" as TryFlipAndBlit's, bit for bit.  `out` =
        caller's arrays to fill instead (any of those four; pageable or page-locked)."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        if out is None:
            shapes = {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "quad_sdr": ((self.fbH, self.fbW, 4, 3), np.float32),
                      "glyphs": ((self.fbH, self.fbW), np.uint16), "rgba": ((2 * self.fbH, self.fbW, 4), np.uint8)}
            want = {"sdr": sdr, "quad_sdr": quad_sdr, "glyphs": glyphs, "rgba": rgba}
            out = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if want[k]}
        p = lambda k, t: out[k].ctypes.data_as(C.POINTER(t)) if out.get(k) is not None else None
        self._r._check(self.L.ycge_video_blit_quadrants(self.ctx, ptr, w, h, bpp, p("sdr", C.c_float), p("quad_sdr", C.c_float), p("glyphs", C.c_uint16),
                                                        p("rgba", C.c_uint8), int(min_contrast)))
        return out

    def TryFlipAndBlitAnsiQuad(self, frame, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                               clear_screen: bool = False, min_contrast: int = 0, sdr: bool = False):
        """TryFlipAndBlitAnsiRgb with quadrant block glyphs (ycge_video_blit_ansi_quad): `bytes`, or (bytes, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_video_blit_ansi_quad, frame, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr, rgb=True,
                               extra=(min_contrast,))

    def TryFlipAndBlitAnsiQuadDelta(self, frame, console_width: int, console_height: int, viewport=(0, 0), default_fg: int = 7, default_bg: int = 0,
                                    clear_screen: bool = False, merge_gap: int = 3, tolerance: int = 0, keyframe: bool = False, min_contrast: int = 0,
                                    sdr: bool = False):
        """The delta form of TryFlipAndBlitAnsiQuad (ycge_video_blit_ansi_quad_delta), on the quadrant family's delta state this context shares
        with RaytraceRenderer.TryFlipAndBlitAnsiQuadDelta: (bytes, info) or (bytes, info, SDR array) with sdr=True."""
        return self._ansi_call(self.L.ycge_video_blit_ansi_quad_delta, frame, console_width, console_height, viewport, default_fg, default_bg, clear_screen, sdr,
                               rgb=True, delta=(merge_gap, tolerance, bool(keyframe), min_contrast))

    # ---------------------------------------------------------------- sixel (ycge_video_blit_pixels / _sixel / _sixel_delta)
    def TryFlipAndBlitPixels(self, frame, rgba: bool = True, index: bool = True, dither: bool = False, sdr: bool = False) -> dict:
        """Every hi-res sample of the blit of `frame` as a pixel (ycge_video_blit_pixels): {name: array} for each output asked - "rgba"
        (2 fbH ss, fbW ss, 4) uint8, the sRGB8 bytes of the Clamp01'd Lanczos sample with alpha 255; "index" (2 fbH ss, fbW ss) uint8, its
        register in the sixel cube (ordered 4 x 4 dither on request); "sdr" as TryFlipAndBlit's, bit for bit.  No state is touched."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        W, H = self.fbW * self.ss, 2 * self.fbH * self.ss
        shapes = {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "rgba": ((H, W, 4), np.uint8), "index": ((H, W), np.uint8)}
        want = {"sdr": sdr, "rgba": rgba, "index": index}
        out = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if want[k]}
        p = lambda k, t: out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        self._r._check(self.L.ycge_video_blit_pixels(self.ctx, ptr, w, h, bpp, p("sdr", C.c_float), p("rgba", C.c_uint8), p("index", C.c_uint8), int(bool(dither))))
        return out

    def TryFlipAndBlitSixel(self, frame, viewport=(0, 0), clear_screen: bool = False, dither: bool = False, sdr: bool = False):
        """The sixel stream of TryFlipAndBlitPixels' registers at cell `viewport` (ycge_video_blit_sixel): `bytes`, or (bytes, SDR array)
        with sdr=True.  The next _delta call of any family returns a keyframe."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        buf, n = self._r._sixel_buffer(), C.c_size_t(0)
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        self._r._check(self.L.ycge_video_blit_sixel(self.ctx, ptr, w, h, bpp, int(viewport[0]), int(viewport[1]), int(bool(clear_screen)), int(bool(dither)),
                                                    buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(n), s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None))
        stream = buf[:n.value].tobytes()
        return (stream, s) if sdr else stream

    def TryFlipAndBlitSixelDelta(self, frame, viewport=(0, 0), clear_screen: bool = False, keyframe: bool = False, dither: bool = False, sdr: bool = False):
        """The delta form of TryFlipAndBlitSixel (ycge_video_blit_sixel_delta), on the delta state this context shares with
        RaytraceRenderer.TryFlipAndBlitSixelDelta: (bytes, info) or (bytes, info, SDR array) with sdr=True.  A still source gives the
        header and the trailer alone."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        buf, n, info = self._r._sixel_buffer(), C.c_size_t(0), (C.c_uint32 * 4)()
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        self._r._check(self.L.ycge_video_blit_sixel_delta(self.ctx, ptr, w, h, bpp, int(viewport[0]), int(viewport[1]), int(bool(clear_screen)), int(bool(keyframe)),
                                                          int(bool(dither)), buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(n), info,
                                                          s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None))
        stream = buf[:n.value].tobytes()
        return (stream, tuple(info), s) if sdr else (stream, tuple(info))

    def TryFlipAndBlitSixelPalette(self, frame, viewport=(0, 0), clear_screen: bool = False, hold: bool = False, sdr: bool = False):
        """The sixel stream of the blit of `frame` under the adaptive palette (ycge_video_blit_sixel_palette), as
        RaytraceRenderer.TryFlipAndBlitSixelPalette: (bytes, palette, count) or (bytes, palette, count, SDR array).  The kept palette is the
        one the context's frames share."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        buf, n = self._r._sixel_palette_buffer(), C.c_size_t(0)
        palette, count = np.zeros((256, 4), np.uint8), C.c_int32(0)
        s = np.zeros((self.fbH, self.fbW, 2, 3), np.float32) if sdr else None
        self._r._check(self.L.ycge_video_blit_sixel_palette(self.ctx, ptr, w, h, bpp, int(viewport[0]), int(viewport[1]), int(bool(clear_screen)), int(bool(hold)),
                                                            buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size, C.byref(n), palette.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                            C.byref(count), s.ctypes.data_as(C.POINTER(C.c_float)) if sdr else None))
        stream = buf[:n.value].tobytes()
        return (stream, palette, count.value, s) if sdr else (stream, palette, count.value)

    def TryFlipAndBlitPixelsPalette(self, frame, rgba: bool = True, index: bool = True, hold: bool = False, sdr: bool = False) -> dict:
        """TryFlipAndBlitPixels' planes with the adaptive palette's registers in "index" (ycge_video_blit_pixels_palette), and "palette"
        (256, 4) uint8 and "count" with them.  The delta state is left alone."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        W, H = self.fbW * self.ss, 2 * self.fbH * self.ss
        shapes = {"sdr": ((self.fbH, self.fbW, 2, 3), np.float32), "rgba": ((H, W, 4), np.uint8), "index": ((H, W), np.uint8), "palette": ((256, 4), np.uint8)}
        want = {"sdr": sdr, "rgba": rgba, "index": index, "palette": True}
        out = {k: np.zeros(shp, dtype=dt) for k, (shp, dt) in shapes.items() if want[k]}
        p = lambda k, t: out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        count = C.c_int32(0)
        self._r._check(self.L.ycge_video_blit_pixels_palette(self.ctx, ptr, w, h, bpp, p("sdr", C.c_float), p("rgba", C.c_uint8), p("index", C.c_uint8), int(bool(hold)),
                                                             p("palette", C.c_uint8), C.byref(count)))
        out["count"] = count.value
        return out

    def pixels_probe(self, frame, fb_width: int, fb_height: int, superSample: int = 1, dither: bool = False):
        """k_video_pixels alone on a caller-given geometry (ycge_test_video_pixels), whatever this console's size: (rgba, index)."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        fn = self.L.ycge_test_video_pixels
        fn.restype, fn.argtypes = abi.SIXEL_DELTA_HOOK_PROTOTYPES["ycge_test_video_pixels"]
        W, H = fb_width * superSample, 2 * fb_height * superSample
        rgba, index = np.zeros((H, W, 4), np.uint8), np.zeros((H, W), np.uint8)
        self._r._check(fn(self.ctx, ptr, w, h, bpp, int(fb_width), int(fb_height), int(superSample), int(bool(dither)), rgba.ctypes.data, index.ctypes.data))
        return rgba, index

    # ---------------------------------------------------------------- tests only
    def blit_quadrants_probe(self, frame, fb_width: int, fb_height: int, superSample: int = 2):
        """k_video_blit_quadrants alone on a caller-given geometry (ycge_test_video_blit_quadrants): (SDR array, sub-cell colours)."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        fn = self.L.ycge_test_video_blit_quadrants
        fn.restype, fn.argtypes = abi.VIDEO_HOOK_PROTOTYPES["ycge_test_video_blit_quadrants"]
        s = np.zeros((fb_height, fb_width, 2, 3), np.float32)
        q = np.zeros((fb_height, fb_width, 4, 3), np.float32)
        self._r._check(fn(self.ctx, f.ctypes.data, w, h, bpp, int(fb_width), int(fb_height), int(superSample), s.ctypes.data, q.ctypes.data))
        return s, q

    def blit_probe(self, frame, fb_width: int, fb_height: int, superSample: int = 1) -> np.ndarray:
        """k_video_blit alone on a caller-given geometry (ycge_test_video_blit), whatever this console's size: the SDR array."""
        f, ptr, w, h, bpp = self._frame_args(frame)
        fn = self.L.ycge_test_video_blit
        fn.restype, fn.argtypes = abi.VIDEO_HOOK_PROTOTYPES["ycge_test_video_blit"]
        s = np.zeros((fb_height, fb_width, 2, 3), np.float32)
        self._r._check(fn(self.ctx, f.ctypes.data, w, h, bpp, int(fb_width), int(fb_height), int(superSample), s.ctypes.data))
        return s


class VolumeCamera:
    """The player of a voxel world as the host keeps it: the body VolumeScene carries between ticks, WorldConfig's three values, and the
    moves of the key events since the last tick.  forward / strafe / rise / jump / shift do HandleInput's arithmetic (Scenes/VolumeScenes.cs:
    169-205: moveSpeed = 6, x ShiftSpeedMult = 30 with Shift held, which also refreshes the fly timer; forwardXZ = (sin yaw, 0, -cos yaw),
    rightXZ = (cos yaw, 0, sin yaw), each times moveSpeed * dt in binary32) and queue a move; tick() hands them to RaytraceRenderer.CameraTick
    with Update's delta time and clears the list."""

    MoveSpeed = np.float32(6.0)
    ShiftSpeedMult = np.float32(30.0)

    def __init__(self, pos, world_height: float, water_level: float, voxel_size_y: float = 1.0, auto_placed: bool = False):
        self.body = abi.CameraBody()
        self.body.pos[:] = [float(np.float32(v)) for v in pos]
        self.body.auto_placed = 1 if auto_placed else 0
        self.world = abi.CameraWorld(float(world_height), float(water_level), float(voxel_size_y))
        self.moves: list = []

    def _speed(self, dt: float, shift_down: bool) -> np.float32:
        dt = max(np.float32(dt), np.float32(0.0))                                   # :167
        speed = self.MoveSpeed
        if shift_down:
            speed = speed * self.ShiftSpeedMult                                        # :175
            self.shift()
        return speed * dt

    def shift(self):
        self.moves.append(abi.CameraMove(abi.CAMERA_MOVE_SHIFT, 0, 0.0, 0.0))

    def forward(self, yaw: float, dt: float, sign: float = 1.0, shift_down: bool = False):
        """W (sign = 1) / S (sign = -1), :198-199"""
        k = self._speed(dt, shift_down)
        sy, cy = np.float32(np.sin(np.float32(yaw))), np.float32(np.cos(np.float32(yaw)))
        s = np.float32(sign)
        self.moves.append(abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, float((s * sy) * k), float((s * -cy) * k)))

    def strafe(self, yaw: float, dt: float, sign: float = 1.0, shift_down: bool = False):
        """D (sign = 1) / A (sign = -1), :200-201"""
        k = self._speed(dt, shift_down)
        sy, cy = np.float32(np.sin(np.float32(yaw))), np.float32(np.cos(np.float32(yaw)))
        s = np.float32(sign)
        self.moves.append(abi.CameraMove(abi.CAMERA_MOVE_HORIZONTAL, 0, float((s * cy) * k), float((s * sy) * k)))

    def rise(self, dt: float, sign: float = 1.0, shift_down: bool = False):
        """E (sign = 1) / Q (sign = -1), :204-205"""
        k = self._speed(dt, shift_down)
        self.moves.append(abi.CameraMove(abi.CAMERA_MOVE_VERTICAL, 0, float(np.float32(sign) * k), 0.0))

    def jump(self, shift_down: bool = False):
        """Space, :208-212"""
        if shift_down:
            self.shift()
        self.moves.append(abi.CameraMove(abi.CAMERA_MOVE_JUMP, 1 if shift_down else 0, 0.0, 0.0))

    def tick(self, renderer: RaytraceRenderer, dt_ms: float, run_update: bool = True) -> dict:
        moves, self.moves = self.moves, []
        return renderer.CameraTick(self.body, self.world, moves, dt_ms, run_update)

    @property
    def pos(self):
        return tuple(self.body.pos)


class VolumeBodies:
    """The bodies of a voxel world that are not the player's alone - mobs, dropped items, projectiles, the other players of a replicated
    scene - ticked together: add() makes a body with its own shape (abi.BodyShape, or None for the reference's 1.7-tall capsule of radius
    0.65) and hands back a VolumeCamera to queue its moves on (forward / strafe / rise / jump / shift); tick() hands every body, its
    shape and its moves to RaytraceRenderer.BodiesTick - one launch for all of them - and clears the lists.  A body whose tick reached a
    cap stays as it was (its moves are dropped with the rest); `results` says which."""

    def __init__(self, world_height: float, water_level: float, voxel_size_y: float = 1.0):
        self.world = abi.CameraWorld(float(world_height), float(water_level), float(voxel_size_y))
        self.bodies: list = []          # VolumeCamera: .body, .moves
        self.shapes: list = []          # abi.BodyShape
        self.results: list = []         # (status, bad_move) of the last tick
        self.infos: list = []

    def add(self, pos, shape=None, auto_placed: bool = False) -> VolumeCamera:
        cam = VolumeCamera(pos, self.world.world_height, self.world.water_level, self.world.voxel_size_y, auto_placed)
        self.bodies.append(cam)
        self.shapes.append(abi.BodyShape(*abi.BODY_SHAPE_DEFAULT) if shape is None else shape if isinstance(shape, abi.BodyShape) else abi.BodyShape(*shape))
        return cam

    def __len__(self):
        return len(self.bodies)

    def tick(self, renderer: RaytraceRenderer, dt_ms: float, run_update: bool = True):
        n = len(self.bodies)
        if n == 0:
            self.results, self.infos = [], []
            return self.results, self.infos
        recs = (abi.CameraBody * n)(*[c.body for c in self.bodies])
        shapes = (abi.BodyShape * n)(*self.shapes)
        self.results, self.infos = renderer.BodiesTick(recs, self.world, [c.moves for c in self.bodies], dt_ms, run_update, shapes)
        for c, r in zip(self.bodies, recs):
            C.memmove(C.byref(c.body), C.byref(r), C.sizeof(abi.CameraBody))
            c.moves = []
        return self.results, self.infos
