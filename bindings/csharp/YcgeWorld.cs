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
}
