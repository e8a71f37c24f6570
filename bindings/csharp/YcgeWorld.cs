// YcgeWorld.cs - ycge_world (include/ycge.h): WorldConfig as a chunk depends on it, for Ycge.ycge_worldgen_chunk_cells and
// Ycge.ycge_scene_generate_grids.  36 bytes, 4-byte aligned: three ints, then WorldMin and VoxelSize.
// HipPregenWorld: the route of a host whose scene is VolumeScenes.BuildMinecraftLike WITH a file name (Ycge.ycge_scene_generate_world).
using System;
using System.Runtime.InteropServices;

namespace ConsoleGame.RayTracing.Native
{
    [StructLayout(LayoutKind.Sequential)]
    public struct YWorld              // ycge_world
    {
        public int ChunkSize;         // 4..64
        public int ChunksY;           // WorldHeight = ChunksY * ChunkSize (WorldConfig.cs:30)
        public int WorldSeed;
        public YVec3 WorldMin;
        public YVec3 VoxelSize;
    }

    /// <summary>BuildMinecraftLike with a world file (VolumeScenes.cs:608-616) builds the whole world with WorldManager.GenerateAndSaveWorld,
    /// reads it back and attaches every chunk.  A host that lets the device do it skips GenerateAndSaveWorld, ReloadFromExistingFile and
    /// EnsureAllChunksLoaded and calls Generate once after its upload: the world is made and attached on the device, and `Index[cx, cy, cz]`
    /// is the device grid of chunk (cx, cy, cz), -1 for a chunk of nothing but Air (AttachChunkFromPreloaded attaches none).  The host shows a
    /// chunk by a YPrim of type VolumeGrid with Ref = that index, in the order it wants Scene.Objects in.</summary>
    public sealed unsafe class HipPregenWorld
    {
        public YWorld World;
        public int ChunksX, ChunksZ;                                  // WorldConfig.ChunksX / ChunksZ; the window starts at block (0, 0) as the reference's
        public int[,,] Index;                                         // [ChunksX, World.ChunksY, ChunksZ] after Generate

        public void Generate(IntPtr ctx, YGrid proto)
        {
            var flat = new int[ChunksX * World.ChunksY * ChunksZ];
            YWorld world = World;
            fixed (int* ix = flat) Ycge.Check(ctx, Ycge.ycge_scene_generate_world(ctx, ref world, ChunksX, ChunksZ, 0, 0, &proto, ix, null));
            Index = new int[ChunksX, World.ChunksY, ChunksZ];
            Buffer.BlockCopy(flat, 0, Index, 0, flat.Length * sizeof(int));
        }

        /// <summary>The same cells on the host, one thread (what GenerateAndSaveWorld would write after the VG01 header).  One managed array:
        /// at most 2^31 - 1 ints, and above 2 GB (the reference's 32 x 8 x 32 chunks of 32 are exactly 2^31 bytes) the runtime needs
        /// gcAllowVeryLargeObjects; a window that does not fit throws before anything is generated.</summary>
        public int[] HostCells()
        {
            long count = 2L * ChunksX * World.ChunkSize * World.ChunksY * World.ChunkSize * ChunksZ * World.ChunkSize;
            if (ChunksX < 1 || ChunksZ < 1 || count <= 0 || count > int.MaxValue) throw new ArgumentOutOfRangeException(nameof(ChunksX), "the window's cells do not fit one int[]");
            var cells = new int[count];
            YWorld world = World;
            fixed (int* c = cells) Ycge.Check(IntPtr.Zero, Ycge.ycge_worldgen_world_cells(ref world, ChunksX, ChunksZ, 0, 0, c));
            return cells;
        }
    }

    /// <summary>A host that HAS a world file (WorldManager.ReloadFromExistingFile) hands its payload over once - or lets the device make the world
    /// (Generate) and writes the file from it (Save) - and then streams by chunk key:
    /// Load makes the cells resident on the device (the header checked as :414-424 checks it), Attach is AttachChunkFromPreloaded for a list
    /// of keys - the slices are cut on the device, no cell crosses the bus again - and returns the device grid per key, -1 for a key outside
    /// the world and for a chunk with no cell of mat != 0 (the reference attaches none).  proto.MinCorner is WorldMin and proto.VoxelSize
    /// is VoxelSize.  The store outlives scene uploads; Release (or ycge_destroy) frees it, and the grids attached from it stay.</summary>
    public sealed unsafe class HipWorldStore
    {
        public int Nx, Ny, Nz, ChunkSize;
        public int ChunksX => (Nx + ChunkSize - 1) / ChunkSize;
        public int ChunksY => (Ny + ChunkSize - 1) / ChunkSize;
        public int ChunksZ => (Nz + ChunkSize - 1) / ChunkSize;

        /// <summary>`file`: the whole VG01 file (a mapped view will do; it is not read after the call).</summary>
        public void Load(IntPtr ctx, byte* file, ulong bytes, int chunkSize)
        {
            int* dims = stackalloc int[3];
            byte* msg = stackalloc byte[256];
            UIntPtr offset;
            if (Ycge.ycge_world_file_info(file, (UIntPtr)bytes, dims, &offset, msg, (UIntPtr)256) != 0)
                throw new System.IO.InvalidDataException(Marshal.PtrToStringAnsi((IntPtr)msg));
            Ycge.Check(ctx, Ycge.ycge_world_store_load(ctx, (int*)(file + (ulong)offset), dims[0], dims[1], dims[2], chunkSize));
            Nx = dims[0]; Ny = dims[1]; Nz = dims[2]; ChunkSize = chunkSize;
        }

        /// <summary>A host that has NO file yet (VolumeScenes.BuildMinecraftLike with a file name that does not exist: GenerateAndSaveWorld, then
        /// ReloadFromExistingFile): the window of chunksX x world.ChunksY x chunksZ chunks at block (0, 0) is made on the device and IS the store -
        /// no cell crosses the bus.  form Ycge.WorldStoreFields keeps the window's 2-D fields (tens of bytes a column) and makes a chunk's cells
        /// when Attach names it; Ycge.WorldStoreCells writes the ordinary cell store on the device.  Attach, Occupied and Release work as after Load.</summary>
        public void Generate(IntPtr ctx, YWorld world, int chunksX, int chunksZ, int form = Ycge.WorldStoreFields)
        {
            Ycge.Check(ctx, Ycge.ycge_world_store_generate(ctx, ref world, chunksX, chunksZ, 0, 0, form));
            ChunkSize = world.ChunkSize;
            Nx = chunksX * ChunkSize; Ny = world.ChunksY * ChunkSize; Nz = chunksZ * ChunkSize;
        }

        /// <summary>The store as a VG01 file (WorldManager.cs:612-629): the header, then the payload in slabs of whole x-planes read back from the
        /// device (at most slabBytes each, one plane at least), so the world never exists in host memory in one piece.</summary>
        public void Save(IntPtr ctx, string path, long slabBytes = 64L << 20)
        {
            long planeInts = 2L * Ny * Nz;
            int per = (int)Math.Max(1, Math.Min(Nx, slabBytes / (planeInts * sizeof(int))));
            var slab = new int[per * planeInts];
            var bytes = new byte[slab.Length * sizeof(int)];
            using (var fs = new System.IO.FileStream(path, System.IO.FileMode.Create, System.IO.FileAccess.Write))
            using (var bw = new System.IO.BinaryWriter(fs))
            {
                bw.Write((byte)'V'); bw.Write((byte)'G'); bw.Write((byte)'0'); bw.Write((byte)'1');
                bw.Write(Nx); bw.Write(Ny); bw.Write(Nz);
                for (int x0 = 0; x0 < Nx; x0 += per)
                {
                    int planes = Math.Min(per, Nx - x0);
                    fixed (int* c = slab) Ycge.Check(ctx, Ycge.ycge_world_store_read(ctx, x0, planes, c));
                    int n = (int)(planes * planeInts * sizeof(int));
                    Buffer.BlockCopy(slab, 0, bytes, 0, n);
                    bw.Write(bytes, 0, n);
                }
            }
        }

        /// <summary>One byte per chunk, [ChunksX, ChunksY, ChunksZ]: 1 when a cell of the chunk has mat != 0 (AttachChunkFromPreloaded's anySolid).</summary>
        public byte[,,] Occupied(IntPtr ctx)
        {
            var flat = new byte[ChunksX * ChunksY * ChunksZ];
            fixed (byte* o = flat) Ycge.Check(ctx, Ycge.ycge_world_store_info(ctx, null, null, o, (UIntPtr)(ulong)flat.Length));
            var occ = new byte[ChunksX, ChunksY, ChunksZ];
            Buffer.BlockCopy(flat, 0, occ, 0, flat.Length);
            return occ;
        }

        /// <summary>keys: {cx, cy, cz} per chunk, in the order the host wants the grids taken (the LoadChunksAround tick: radial, then cy).</summary>
        public int[] Attach(IntPtr ctx, int[] keys, YGrid proto)
        {
            var index = new int[keys.Length / 3];
            fixed (int* k = keys) fixed (int* ix = index) Ycge.Check(ctx, Ycge.ycge_scene_attach_world_chunks(ctx, k, index.Length, &proto, ix));
            return index;
        }

        /// <summary>A store generated with Ycge.WorldStoreFields takes edits (HipVoxelEdits.ApplyToStore) only with a pool of materialised
        /// chunks: maxChunks slots of ChunkSize^3 cells, 8 bytes a cell, on every device.  Every chunk an op touches takes a slot and keeps it
        /// until RevertChunks; an edit that needs more slots than are free is refused as a whole (YCGE_ERR_OUT_OF_MEMORY).  A later call with a
        /// larger count grows the pool.  Release, Load and Generate drop it.</summary>
        public void ReserveEdits(IntPtr ctx, int maxChunks) { Ycge.Check(ctx, Ycge.ycge_world_store_reserve_edits(ctx, maxChunks)); }

        /// <summary>{slots of the pool, slots that hold a chunk}; {0, 0} for a store without a pool.</summary>
        public int[] EditSlots(IntPtr ctx)
        {
            var s = new int[2];
            fixed (int* p = s) Ycge.Check(ctx, Ycge.ycge_world_store_edit_slots(ctx, p, p + 1));
            return s;
        }

        /// <summary>keys: {cx, cy, cz} per chunk.  Their slots are free again and each chunk is the generated chunk once more.</summary>
        public void RevertChunks(IntPtr ctx, int[] keys)
        {
            fixed (int* k = keys) Ycge.Check(ctx, Ycge.ycge_world_store_revert_chunks(ctx, k, keys.Length / 3));
        }

        public void Release(IntPtr ctx) { Ycge.Check(ctx, Ycge.ycge_world_store_release(ctx)); Nx = Ny = Nz = 0; }
    }

    /// <summary>A host's SetBlock: boxes of one (matId, metaId) pair written into resident grids (ycge_scene_edit_voxels) and into the world
    /// store (ycge_world_store_edit) where they lie - no cell of the world has to exist in host memory.  Ops apply in list order; where
    /// boxes overlap the later op wins.  A refused list changes nothing (Ycge.Check throws with the message, which names the op).  On a grid
    /// the host encoded (a grid of the upload; a lookup table above 254 entries) a 256th distinct pair is refused with YCGE_ERR_UNSUPPORTED:
    /// codes are not reclaimed, detach the grid and attach it again.</summary>
    public sealed unsafe class HipVoxelEdits
    {
        readonly System.Collections.Generic.List<YVoxelEdit> ops = new System.Collections.Generic.List<YVoxelEdit>();
        public int Count => ops.Count;
        public void Clear() { ops.Clear(); }

        /// <summary>gridIndex: the device grid (0 for a store edit); the box is inclusive, in the grid's - or the store's - cell indices.</summary>
        public void Box(int gridIndex, int x0, int y0, int z0, int x1, int y1, int z1, int matId, int metaId)
        {
            var e = new YVoxelEdit { GridIndex = gridIndex, MatId = matId, MetaId = metaId };
            e.Lo[0] = x0; e.Lo[1] = y0; e.Lo[2] = z0; e.Hi[0] = x1; e.Hi[1] = y1; e.Hi[2] = z1;
            ops.Add(e);
        }
        public void Cell(int gridIndex, int x, int y, int z, int matId, int metaId) { Box(gridIndex, x, y, z, x, y, z, matId, metaId); }

        /// <summary>{cells whose code changed, bricks written, grids whose record changed, objects installed again (0 or 1)}.  The scene is
        /// complete afterwards: no ycge_scene_update_objects has to follow.</summary>
        public uint[] ApplyToScene(IntPtr ctx)
        {
            var info = new uint[4];
            var list = ops.ToArray();
            fixed (YVoxelEdit* o = list) fixed (uint* i = info) Ycge.Check(ctx, Ycge.ycge_scene_edit_voxels(ctx, o, list.Length, i));
            return info;
        }

        /// <summary>The same list, in store cell coordinates, into the context's world store (every GridIndex 0).</summary>
        public void ApplyToStore(IntPtr ctx)
        {
            var list = ops.ToArray();
            fixed (YVoxelEdit* o = list) Ycge.Check(ctx, Ycge.ycge_world_store_edit(ctx, o, list.Length));
        }
    }
}
