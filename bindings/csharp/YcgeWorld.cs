// YcgeWorld.cs - ycge_world (include/ycge.h): WorldConfig as a chunk depends on it, for Ycge.ycge_worldgen_chunk_cells and
// Ycge.ycge_scene_generate_grids.  36 bytes, 4-byte aligned: three ints, then WorldMin and VoxelSize.
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
}
