// HipObjLoader.cs - MeshLoader.FromObj and MeshScenes.AddMeshAutoGround with the file read on the GPU (ycge_obj_parse, include/ycge.h).
//
// The reference's host parses every mesh file on one thread (StreamReader.ReadLine, String.Split, float.Parse per token) and, for an
// auto-grounded mesh, parses it twice: TryReadObjBoundsNormalized reads the same file again before FromObj does.  Here the file's bytes go
// up once; FromObj is ycge_obj_parse + ycge_obj_triangles, and AddMeshAutoGround reads positions and faces back once (ycge_obj_read) for
// the part of TryReadObjBoundsNormalized that stays on the host - largest connected component by union-find, the serial centroid sum,
// the centred bounds - and then asks the device for the placed triangles.  The floats are the ones float.Parse gives (.NET Core 3.0 and
// later: correctly rounded to binary32); the files the library refuses are listed in INTEGRATION.md.
// The triangles come back as the float soup ycge_mesh.triangles takes (9 per triangle: A, B, C) with the mesh bounds.
using System;
using System.IO;
using ConsoleGame.RayTracing.Native;

namespace ConsoleGame.RayTracing
{
    public sealed unsafe class HipObjMesh
    {
        public float[] Triangles;          // 9 per triangle
        public float[] Bounds;             // min xyz, max xyz
        public int TriangleCount => Triangles.Length / 9;
        public bool ParsedOnDevice;
    }

    public static unsafe class HipObjLoader
    {
        /// <summary>MeshLoader.FromObj(path, ..., scale, translate, normalize, targetSize) through the context `ctx` (any context: no scene is needed or touched).</summary>
        public static HipObjMesh FromObj(IntPtr ctx, string path, float scale = 1.0f, float tx = 0.0f, float ty = 0.0f, float tz = 0.0f, bool normalize = true, float targetSize = 1.0f)
        {
            YObjInfo info = Parse(ctx, path);
            try { return Triangles(ctx, info, normalize, targetSize, scale, tx, ty, tz); }
            finally { Ycge.ycge_obj_release(ctx); }
        }

        /// <summary>MeshScenes.AddMeshAutoGround: the mesh normalised to extent 1, scaled, and set on the ground at targetPos - one parse.</summary>
        public static HipObjMesh AddMeshAutoGround(IntPtr ctx, string path, float scale, float targetX, float targetY, float targetZ)
        {
            YObjInfo info = Parse(ctx, path);
            try
            {
                float[] pos = new float[3 * info.NPositions];
                int[] faces = new int[3 * info.NTriangles];
                fixed (float* pp = pos) fixed (int* pf = faces) Ycge.Check(ctx, Ycge.ycge_obj_read(ctx, pp, pf));
                if (!BoundsOfLargestComponentNormalized(pos, faces, out float minYNormalized)) throw new FileNotFoundException("OBJ not found or empty", path);
                float yTranslate = targetY - minYNormalized * scale + 0.01f;
                return Triangles(ctx, info, true, 1.0f, scale, targetX, yTranslate, targetZ);
            }
            finally { Ycge.ycge_obj_release(ctx); }
        }

        private static YObjInfo Parse(IntPtr ctx, string path)
        {
            if (string.IsNullOrWhiteSpace(path)) throw new ArgumentException("path");
            if (!File.Exists(path)) throw new FileNotFoundException("OBJ not found", path);
            byte[] text = File.ReadAllBytes(path);
            YObjInfo info;
            fixed (byte* p = text) Ycge.Check(ctx, Ycge.ycge_obj_parse(ctx, p, (UIntPtr)(ulong)text.Length, out info));
            return info;
        }

        private static HipObjMesh Triangles(IntPtr ctx, YObjInfo info, bool normalize, float targetSize, float scale, float tx, float ty, float tz)
        {
            var mesh = new HipObjMesh { Triangles = new float[9 * info.NTriangles], Bounds = new float[6], ParsedOnDevice = info.OnDevice != 0 };
            float* t = stackalloc float[3];
            t[0] = tx; t[1] = ty; t[2] = tz;
            fixed (float* pt = mesh.Triangles) fixed (float* pb = mesh.Bounds)
                Ycge.Check(ctx, Ycge.ycge_obj_triangles(ctx, normalize ? 1 : 0, targetSize, scale, t, pt, pb));
            return mesh;
        }

        // The host part of MeshScenes.TryReadObjBoundsNormalized (MeshScenes.cs:233-330) on parsed arrays: the component with the most faces
        // (the first such one in the order its faces appear), its centroid as the running binary32 sum of (A + B + C) * (1/3f) over its faces
        // times 1 / faces, the bounds of its vertices about that centroid, divided by their largest extent.  Only min.Y is needed here.
        private static bool BoundsOfLargestComponentNormalized(float[] pos, int[] faces, out float minY)
        {
            minY = 0.0f;
            int nv = pos.Length / 3, nf = faces.Length / 3;
            if (nv == 0 || nf == 0) return false;
            int[] parent = new int[nv];
            byte[] rank = new byte[nv];
            for (int i = 0; i < nv; i++) parent[i] = i;
            int Find(int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; }
            void Union(int x, int y)
            {
                int a = Find(x), b = Find(y);
                if (a == b) return;
                if (rank[a] < rank[b]) parent[a] = b;
                else { parent[b] = a; if (rank[a] == rank[b]) rank[a]++; }
            }
            for (int f = 0; f < nf; f++) { Union(faces[3 * f], faces[3 * f + 1]); Union(faces[3 * f + 1], faces[3 * f + 2]); }
            // faces per component root; the winner is the first root, in order of first appearance, with the strictly largest count
            int[] count = new int[nv];
            int[] firstSeen = new int[nv];
            int[] rootOf = new int[nf];
            int seen = 0;
            for (int f = 0; f < nf; f++) { int r = Find(faces[3 * f]); rootOf[f] = r; if (count[r]++ == 0) firstSeen[r] = seen++; }
            int best = -1;
            for (int f = 0; f < nf; f++)
            {
                int r = rootOf[f];
                if (best == -1 || count[r] > count[best] || (count[r] == count[best] && firstSeen[r] < firstSeen[best])) best = r;
            }
            float cx = 0.0f, cy = 0.0f, cz = 0.0f;
            const float third = 1.0f / 3.0f;
            bool[] used = new bool[nv];
            for (int f = 0; f < nf; f++)
            {
                if (rootOf[f] != best) continue;
                int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
                used[a] = used[b] = used[c] = true;
                cx += (pos[3 * a] + pos[3 * b] + pos[3 * c]) * third;
                cy += (pos[3 * a + 1] + pos[3 * b + 1] + pos[3 * c + 1]) * third;
                cz += (pos[3 * a + 2] + pos[3 * b + 2] + pos[3 * c + 2]) * third;
            }
            float inv = 1.0f / count[best];
            cx *= inv; cy *= inv; cz *= inv;
            float loX = float.PositiveInfinity, loY = float.PositiveInfinity, loZ = float.PositiveInfinity;
            float hiX = float.NegativeInfinity, hiY = float.NegativeInfinity, hiZ = float.NegativeInfinity;
            for (int v = 0; v < nv; v++)
            {
                if (!used[v]) continue;
                float x = pos[3 * v] - cx, y = pos[3 * v + 1] - cy, z = pos[3 * v + 2] - cz;
                if (x < loX) loX = x; if (y < loY) loY = y; if (z < loZ) loZ = z;
                if (x > hiX) hiX = x; if (y > hiY) hiY = y; if (z > hiZ) hiZ = z;
            }
            float extent = hiX - loX;
            if (hiY - loY > extent) extent = hiY - loY;
            if (hiZ - loZ > extent) extent = hiZ - loZ;
            if (extent <= 0.0f) extent = 1.0f;
            minY = loY * (1.0f / extent);
            return true;
        }
    }
}
