"""Host-side mirror of the reference's voxel world file and chunk attachment.

Reference: ConsoleGame/RayTracing/Scenes/WorldGeneration/WorldManager.cs
  * `VG01` file: writer :612-629, reader ReloadFromExistingFile :399-441 — 4 header bytes 'V','G','0','1'
    (BinaryWriter.Write(char) = one UTF-8 byte each), int32 nx, ny, nz (little endian), then for x, y, z
    (z fastest) the pair int32 matId, int32 metaId.  That is exactly the cell order `ycge_grid.cells` takes.
  * BuildDesiredSet :372-397 — the chunk keys within ViewDistanceChunks of the camera column, every cy.
  * AttachChunkFromPreloaded :696-731 — slice a chunk out of the preloaded world, skip it when it is all air,
    place it at WorldMin + c * ChunkSize * VoxelSize.

Setup code on the data side of the hot path: it produces the VolumeGrid objects `Scene.Objects` holds; all
arithmetic that reaches the tracer is binary32, operation for operation as in the C#.
"""
from __future__ import annotations

import math
import struct
from typing import Callable, Iterable, List, Optional, Tuple

import numpy as np

from .scene import Scene, VolumeGrid, vec3

f32 = np.float32
MAGIC = b"VG01"


def write_vg01(path, cells: np.ndarray) -> None:
    """cells: int32 [nx, ny, nz, 2] = (matId, metaId).  WorldManager.cs:612-629."""
    c = np.ascontiguousarray(cells, dtype="<i4")
    if c.ndim != 4 or c.shape[3] != 2:
        raise ValueError("cells must be [nx, ny, nz, 2]")
    nx, ny, nz = c.shape[:3]
    with open(path, "wb") as fh:
        fh.write(MAGIC)
        fh.write(struct.pack("<iii", nx, ny, nz))
        fh.write(c.tobytes())


def read_vg01(path) -> np.ndarray:
    """Returns int32 [nx, ny, nz, 2].  Error behaviour of ReloadFromExistingFile (:399-441): missing file ->
    FileNotFoundError, bad header / dimensions -> ValueError (InvalidDataException), short file -> EOFError."""
    if path is None or str(path).strip() == "":
        raise ValueError("filename is null or empty.")
    with open(path, "rb") as fh:
        head = fh.read(4)
        if head != MAGIC:
            raise ValueError("Unsupported world file header. Expected 'VG01'.")
        dims = fh.read(12)
        if len(dims) < 12:
            raise EOFError("Unable to read beyond the end of the stream.")
        nx, ny, nz = struct.unpack("<iii", dims)
        if nx <= 0 or ny <= 0 or nz <= 0:
            raise ValueError("Invalid world dimensions.")
        want = nx * ny * nz * 8
        data = fh.read(want)
        if len(data) < want:
            raise EOFError("Unable to read beyond the end of the stream.")
    return np.frombuffer(data, dtype="<i4").reshape(nx, ny, nz, 2).copy()


def pregen_world(lib, world, chunks_x: int, chunks_z: int, path=None, origin=(0, 0)) -> np.ndarray:
    """GenerateAndSaveWorld (WorldManager.cs:510-631) by the library's host generator (ycge_worldgen_world_cells; `lib` the loaded
    library, `world` an abi.World): the cells [nx, ny, nz, 2] of the window, written as a VG01 file when `path` is given."""
    import ctypes as C
    S = int(world.chunk_size)
    cells = np.zeros((chunks_x * S, int(world.chunks_y) * S, chunks_z * S, 2), np.int32)
    rc = lib.ycge_worldgen_world_cells(C.byref(world), chunks_x, chunks_z, int(origin[0]), int(origin[1]), cells.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise ValueError(f"ycge_worldgen_world_cells refused the window (status {rc})")
    if path is not None:
        write_vg01(path, cells)
    return cells


SAVE_SLAB_BYTES = 64 << 20          # save_resident's default slab: the payload a host holds at one time


def save_resident(renderer, path, slab_planes: Optional[int] = None) -> Tuple[int, int, int]:
    """The renderer's resident world (LoadWorld or GenerateWorldStore) written as a VG01 file (WorldManager.cs:612-629): the header, then the
    payload in slabs of `slab_planes` x-planes read back by RaytraceRenderer.ReadWorldCells (ycge_world_store_read) - by default what
    SAVE_SLAB_BYTES holds, one plane at least - so a 2 GB world never exists in host memory in one piece.  Returns (nx, ny, nz)."""
    (nx, ny, nz), _, _ = renderer.WorldInfo()
    if slab_planes is None:
        slab_planes = SAVE_SLAB_BYTES // (8 * ny * nz)
    slab_planes = max(1, min(int(slab_planes), nx))
    with open(path, "wb") as fh:
        fh.write(MAGIC)
        fh.write(struct.pack("<iii", nx, ny, nz))
        for x0 in range(0, nx, slab_planes):
            fh.write(np.ascontiguousarray(renderer.ReadWorldCells(x0, min(slab_planes, nx - x0)), dtype="<i4").data)
    return nx, ny, nz


def pregen_resident(renderer, world, chunks_x: int, chunks_z: int, path=None, origin=(0, 0), form="fields", edit_chunks: Optional[int] = None) -> Tuple[int, int, int]:
    """pregen_world's counterpart on the device: GenerateAndSaveWorld (WorldManager.cs:510-631) as RaytraceRenderer.GenerateWorldStore - the
    window becomes the renderer's resident world, ready for stream_resident / load_all_resident - written as a VG01 file slab by slab
    (save_resident) when `path` is given.  No array of the world is made on the host.  `edit_chunks`: a fields store is given a pool of
    that many materialised chunks (RaytraceRenderer.ReserveWorldEdits), so edit_resident works on it.  Returns (nx, ny, nz)."""
    dims = renderer.GenerateWorldStore(world, chunks_x, chunks_z, origin=origin, form=form)
    if edit_chunks is not None:
        renderer.ReserveWorldEdits(edit_chunks)
    if path is not None:
        save_resident(renderer, path)
    return dims


def center_column(center, world_min, voxel_size, chunk_size: int) -> Tuple[int, int]:
    """(cxCenter, czCenter) of BuildDesiredSet / LoadChunksAround (WorldManager.cs:309-312, 376-379), in binary32 as there."""
    scale_x = f32(f32(voxel_size[0]) * f32(chunk_size))
    scale_z = f32(f32(voxel_size[2]) * f32(chunk_size))
    return (int(math.floor(float(f32((f32(center[0]) - f32(world_min[0])) / scale_x)))),
            int(math.floor(float(f32((f32(center[2]) - f32(world_min[2])) / scale_z)))))


def build_desired_set(center, world_min, voxel_size, chunk_size: int, view_distance_chunks: int, chunks_y: int) -> List[Tuple[int, int, int]]:
    """BuildDesiredSet, WorldManager.cs:372-397.  Returned in insertion order (cx, then cz, then cy), which is
    the order EnsureViewLoaded (:634-656) attaches chunks in - and so the order of Scene.Objects."""
    scale_x = f32(f32(voxel_size[0]) * f32(chunk_size))
    scale_z = f32(f32(voxel_size[2]) * f32(chunk_size))
    cx_center = int(math.floor(float(f32((f32(center[0]) - f32(world_min[0])) / scale_x))))
    cz_center = int(math.floor(float(f32((f32(center[2]) - f32(world_min[2])) / scale_z))))
    out = []
    for cx in range(cx_center - view_distance_chunks, cx_center + view_distance_chunks + 1):
        for cz in range(cz_center - view_distance_chunks, cz_center + view_distance_chunks + 1):
            for cy in range(chunks_y):
                out.append((cx, cy, cz))
    return out


def slice_chunk(world: np.ndarray, cx: int, cy: int, cz: int, chunk_size: int) -> Optional[np.ndarray]:
    """The cells of chunk (cx, cy, cz), clipped at the world's far faces; None when outside or all air (:698-718)."""
    nx, ny, nz = world.shape[:3]
    if cx < 0 or cy < 0 or cz < 0:
        return None             # the C# would index out of range; the reference never asks (keys are clamped by its callers)
    sx, sy, sz = min(chunk_size, nx - cx * chunk_size), min(chunk_size, ny - cy * chunk_size), min(chunk_size, nz - cz * chunk_size)
    if sx <= 0 or sy <= 0 or sz <= 0:
        return None
    cells = world[cx * chunk_size:cx * chunk_size + sx, cy * chunk_size:cy * chunk_size + sy, cz * chunk_size:cz * chunk_size + sz]
    if not (cells[..., 0] != 0).any():
        return None
    return np.ascontiguousarray(cells)


def chunk_min_corner(world_min, voxel_size, chunk_size: int, cx: int, cy: int, cz: int):
    """:720-724: WorldMin + c * ChunkSize * VoxelSize, evaluated left to right in binary32 (int * int first)."""
    return vec3(f32(world_min[0]) + f32(cx * chunk_size) * f32(voxel_size[0]),
                f32(world_min[1]) + f32(cy * chunk_size) * f32(voxel_size[1]),
                f32(world_min[2]) + f32(cz * chunk_size) * f32(voxel_size[2]))


def attach_view(scene: Scene, world: np.ndarray, center, world_min, voxel_size, chunk_size: int, view_distance_chunks: int,
                material_lookup: Callable, chunks_y: Optional[int] = None, loaded: Optional[dict] = None) -> List[Tuple[int, int, int]]:
    """EnsureViewLoaded over a preloaded world (:634-656): attaches every desired, not yet loaded, non-air chunk to
    scene.Objects in desired-set order.  `loaded` (key -> VolumeGrid) persists between calls like loadedChunkMap."""
    if chunks_y is None:
        chunks_y = (world.shape[1] + chunk_size - 1) // chunk_size
    loaded = {} if loaded is None else loaded
    added = []
    for key in build_desired_set(center, world_min, voxel_size, chunk_size, view_distance_chunks, chunks_y):
        if key in loaded:
            continue
        cells = slice_chunk(world, *key, chunk_size)
        if cells is None:
            continue
        vg = VolumeGrid(cells, chunk_min_corner(world_min, voxel_size, chunk_size, *key), vec3(*voxel_size), material_lookup)
        loaded[key] = vg
        scene.Objects.append(vg)
        added.append(key)
    return added


def stream_view(scene: Scene, world: np.ndarray, center, world_min, voxel_size, chunk_size: int, view_distance_chunks: int,
                material_lookup: Callable, loaded: dict, chunks_y: Optional[int] = None, cache: Optional[dict] = None):
    """One LoadChunksAround tick over a preloaded world (WorldManager.cs:289-370): loaded chunks outside the new desired set leave
    scene.Objects (:341-363; into `cache` when one is given, as CacheChunk does), the desired chunks that are not loaded are attached in
    the reference's order - radial distance from the centre column, then cy (:313-320; the sort is stable over the desired set's
    insertion order) - from `cache` when they are there (TryAttachFromCache).  `loaded` (key -> VolumeGrid) persists between calls like
    loadedChunkMap.  Returns (added keys, removed keys)."""
    if chunks_y is None:
        chunks_y = (world.shape[1] + chunk_size - 1) // chunk_size
    desired = build_desired_set(center, world_min, voxel_size, chunk_size, view_distance_chunks, chunks_y)
    want = set(desired)
    removed = [key for key in loaded if key not in want]
    for key in removed:
        vg = loaded.pop(key)
        for i, o in enumerate(scene.Objects):
            if o is vg:
                del scene.Objects[i]
                break
        if cache is not None:
            cache[key] = vg
    cx0, cz0 = center_column(center, world_min, voxel_size, chunk_size)
    todo = [key for key in desired if key not in loaded]
    todo.sort(key=lambda k: ((k[0] - cx0) * (k[0] - cx0) + (k[2] - cz0) * (k[2] - cz0), k[1]))
    added = []
    for key in todo:
        vg = cache.pop(key, None) if cache is not None else None
        if vg is None:
            cells = slice_chunk(world, *key, chunk_size)
            if cells is None:
                continue
            vg = VolumeGrid(cells, chunk_min_corner(world_min, voxel_size, chunk_size, *key), vec3(*voxel_size), material_lookup)
        loaded[key] = vg
        scene.Objects.append(vg)
        added.append(key)
    return added, removed


def stream_generated(renderer, world, proto, center, view_distance_chunks: int, loaded: dict):
    """One LoadChunksAround tick with no world file behind it (WorldManager.cs:289-370 with AttachChunkFromGenerator, :754-793): the
    desired chunks that are not loaded are GENERATED ON THE DEVICE and attached (RaytraceRenderer.GenerateGrids, ycge_scene_generate_grids)
    in the reference's order; the keys that left the view are returned for the caller to drop from its object list and detach.  `world`
    is an abi.World, `proto` the abi.Grid whose lookup serves every chunk; `loaded` (key -> device grid index, -1 for an all-air chunk)
    persists between calls.  Returns (added keys, removed keys, indices of the removed resident grids)."""
    wmin = (world.world_min.x, world.world_min.y, world.world_min.z)
    vox = (world.voxel_size.x, world.voxel_size.y, world.voxel_size.z)
    desired = build_desired_set(center, wmin, vox, world.chunk_size, view_distance_chunks, world.chunks_y)
    want = set(desired)
    removed = [key for key in loaded if key not in want]
    gone = [loaded.pop(key) for key in removed]
    cx0, cz0 = center_column(center, wmin, vox, world.chunk_size)
    todo = [key for key in desired if key not in loaded]
    todo.sort(key=lambda k: ((k[0] - cx0) * (k[0] - cx0) + (k[2] - cz0) * (k[2] - cz0), k[1]))
    if todo:
        for key, i in zip(todo, renderer.GenerateGrids(world, todo, proto)):
            loaded[key] = i
    return todo, removed, [i for i in gone if i >= 0]


def stream_resident(renderer, proto, center, chunk_size: int, view_distance_chunks: int, chunks_y: int, loaded: dict):
    """One LoadChunksAround tick over a world that is RESIDENT ON THE DEVICE (RaytraceRenderer.LoadWorld): stream_view's tick - the same
    desired set, the same radial-then-cy order - with AttachChunkFromPreloaded done by the device (RaytraceRenderer.AttachWorldChunks,
    ycge_scene_attach_world_chunks): no cell is sliced or sent by the host.  `proto` is the abi.Grid whose min_corner is WorldMin, whose
    voxel_size is VoxelSize and whose lookup serves every chunk; `loaded` (key -> device grid index, -1 for a chunk that took no slot: all
    air, or outside the world) persists between calls.  Returns (added keys, removed keys, indices of the removed resident grids), as
    stream_generated does, for the caller to update its objects and detach."""
    wmin = (proto.min_corner.x, proto.min_corner.y, proto.min_corner.z)
    vox = (proto.voxel_size.x, proto.voxel_size.y, proto.voxel_size.z)
    desired = build_desired_set(center, wmin, vox, chunk_size, view_distance_chunks, chunks_y)
    want = set(desired)
    removed = [key for key in loaded if key not in want]
    gone = [loaded.pop(key) for key in removed]
    cx0, cz0 = center_column(center, wmin, vox, chunk_size)
    todo = [key for key in desired if key not in loaded]
    todo.sort(key=lambda k: ((k[0] - cx0) * (k[0] - cx0) + (k[2] - cz0) * (k[2] - cz0), k[1]))
    if todo:
        for key, i in zip(todo, renderer.AttachWorldChunks(todo, proto)):
            loaded[key] = i
    return todo, removed, [i for i in gone if i >= 0]


def clip_ops_to_chunks(ops, keys: Iterable[Tuple[int, int, int]], chunk_size: int) -> dict:
    """World-coordinate edit ops (int [n, 9]: {0, lo xyz, hi xyz, mat_id, meta_id}, ycge_voxel_edit rows with grid_index 0) cut to the chunks
    `keys`: {key: int32 [m, 8] = {lo xyz, hi xyz, mat_id, meta_id} in the chunk's own cell indices, in list order} for every key a box
    intersects.  A chunk's far faces need no clipping of their own: a box inside the world ends where the world ends."""
    ops = np.asarray(ops, np.int64).reshape(-1, 9)
    out = {}
    for key in keys:
        base = np.asarray(key, np.int64) * chunk_size
        rows = []
        for op in ops:
            lo, hi = np.maximum(op[1:4], base), np.minimum(op[4:7], base + chunk_size - 1)
            if (lo <= hi).all():
                rows.append([*(lo - base), *(hi - base), op[7], op[8]])
        if rows:
            out[tuple(int(v) for v in key)] = np.asarray(rows, np.int32)
    return out


def edit_resident(renderer, ops, loaded: dict, chunk_size: int, proto=None):
    """The SetBlock a host would write over a world that is resident on the device: the world-coordinate `ops` (int [n, 9], rows of
    {0, lo xyz, hi xyz, mat_id, meta_id}; list order, the later op wins) go to the world store (RaytraceRenderer.EditWorldCells) and, clipped
    and translated to chunk-local boxes, to every loaded chunk they intersect (RaytraceRenderer.EditVoxels, one call) - afterwards the
    resident grids and the store agree, and no cell crossed the bus.  `loaded` is stream_resident's map (key -> device grid index, -1 for
    a chunk in view that took no slot); a chunk in view that the edit makes occupied is attached from the store when `proto` (the
    abi.Grid of stream_resident) is given, and its index entered.  Returns (EditVoxels' info or None when no loaded chunk was touched,
    the keys attached); the caller shows a new chunk with its next object list, as after stream_resident."""
    ops = np.asarray(ops, np.int64).reshape(-1, 9)
    renderer.EditWorldCells(ops)
    local = clip_ops_to_chunks(ops, [k for k, i in loaded.items() if i >= 0], chunk_size)
    rows = [[loaded[key], *r] for key, boxes in local.items() for r in boxes]
    info = renderer.EditVoxels(np.asarray(rows, np.int64)) if rows else None
    attached = []
    if proto is not None:
        _, _, occupied = renderer.WorldInfo()
        inside = lambda k: all(0 <= k[a] < occupied.shape[a] for a in range(3))
        todo = [k for k in clip_ops_to_chunks(ops, [k for k, i in loaded.items() if i < 0 and inside(k)], chunk_size) if occupied[k]]
        for key, i in zip(todo, renderer.AttachWorldChunks(todo, proto) if todo else []):
            loaded[key] = i
            attached.append(key)
    return info, attached


def load_all_order(dims, chunk_size: int, center, world_min, voxel_size) -> List[Tuple[int, int, int]]:
    """The keys of every chunk of a world of `dims` cells in the order ReloadFromExistingFile queues them (WorldManager.cs:447-480): by
    squared distance of (cx, cz) from the centre column - clamped into the world, :465-468 - then cy.  The C# sort is not stable and starts
    from a HashSet's order, so keys that tie are in no defined order there; here they keep (cx, cy, cz) order."""
    counts = [(int(d) + chunk_size - 1) // chunk_size for d in dims]
    cx0 = int(math.floor(float(f32((float(center[0]) - float(world_min[0])) / (float(voxel_size[0]) * chunk_size)))))
    cz0 = int(math.floor(float(f32((float(center[2]) - float(world_min[2])) / (float(voxel_size[2]) * chunk_size)))))
    cx0, cz0 = min(max(cx0, 0), counts[0] - 1), min(max(cz0, 0), counts[2] - 1)
    keys = [(cx, cy, cz) for cx in range(counts[0]) for cy in range(counts[1]) for cz in range(counts[2])]
    keys.sort(key=lambda k: ((k[0] - cx0) * (k[0] - cx0) + (k[2] - cz0) * (k[2] - cz0), k[1]))
    return keys


def load_all_resident(renderer, proto, center, loaded: Optional[dict] = None):
    """ReloadFromExistingFile's attach of the whole file (:447-508) over the renderer's resident world: every chunk in load_all_order's
    order, one AttachWorldChunks call.  Returns (keys in that order, their device indices: -1 for an all-air chunk); `loaded`, when given,
    receives key -> index as stream_resident keeps it."""
    dims, chunk_size, _ = renderer.WorldInfo()
    wmin = (proto.min_corner.x, proto.min_corner.y, proto.min_corner.z)
    vox = (proto.voxel_size.x, proto.voxel_size.y, proto.voxel_size.z)
    keys = load_all_order(dims, chunk_size, center, wmin, vox)
    idx = renderer.AttachWorldChunks(keys, proto)
    if loaded is not None:
        loaded.update(zip(keys, idx))
    return keys, idx
