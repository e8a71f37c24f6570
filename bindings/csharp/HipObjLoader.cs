// HipObjLoader.cs - MeshLoader.FromObj and MeshScenes.AddMeshAutoGround with the file read on the GPU (ycge_obj_parse, include/ycge.h).
//
// The reference's host parses every mesh file on one thread (StreamReader.ReadLine, String.Split, float.Parse per token) and, for an
// auto-grounded mesh, parses it twice: TryReadObjBoundsNormalized reads the same file again before FromObj does.  Here the file's bytes go
// up once; FromObj is ycge_obj_parse + ycge_obj_triangles, and AddMeshAutoGround is ycge_obj_parse + ycge_obj_triangles_auto_ground: the
// rest of TryReadObjBoundsNormalized - largest connected component, the serial centroid sum, the centred bounds - runs on the device
// against the held OBJ (the library's own host tail is its fallback), the yTranslate arithmetic happens in the library, and no geometry
// comes back before the placed triangles.  The floats are the ones float.Parse gives (.NET Core 3.0 and later: correctly rounded to
// binary32); the files the library refuses are listed in INTEGRATION.md.
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
        public bool GroundedOnDevice;      // AddMeshAutoGround: the kernels found the component, its centroid and bounds
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
                var mesh = new HipObjMesh { Triangles = new float[9 * info.NTriangles], Bounds = new float[6], ParsedOnDevice = info.OnDevice != 0 };
                float* t = stackalloc float[3];
                t[0] = targetX; t[1] = targetY; t[2] = targetZ;
                YObjGroundInfo ground;
                fixed (float* pt = mesh.Triangles) fixed (float* pb = mesh.Bounds)
                    Ycge.Check(ctx, Ycge.ycge_obj_triangles_auto_ground(ctx, scale, t, pt, pb, &ground));
                mesh.GroundedOnDevice = ground.OnDevice != 0;
                return mesh;
            }
            finally { Ycge.ycge_obj_release(ctx); }
        }

        /// <summary>The OBJ at `path` added to the RESIDENT scene of `ctx` as a mesh of material index `material` (ycge_scene_attach_obj_mesh):
        /// placed as FromObj places it - or, with autoGround, as AddMeshAutoGround at (tx, ty, tz) - and handed to the tree builder where the
        /// OBJ kernels wrote it; no triangle comes back.  Returns the device mesh index (ycge_prim.ref of the next ycge_scene_update_objects);
        /// bounds: min xyz, max xyz.</summary>
        public static int AttachToScene(IntPtr ctx, string path, int material, out float[] bounds, float scale = 1.0f, float tx = 0.0f, float ty = 0.0f, float tz = 0.0f,
                                        bool normalize = true, float targetSize = 1.0f, bool autoGround = false)
        {
            Parse(ctx, path);
            try
            {
                bounds = new float[6];
                float* t = stackalloc float[3];
                t[0] = tx; t[1] = ty; t[2] = tz;
                int index;
                fixed (float* pb = bounds)
                    Ycge.Check(ctx, Ycge.ycge_scene_attach_obj_mesh(ctx, autoGround ? 1 : 0, normalize ? 1 : 0, targetSize, scale, t, material, &index, pb));
                return index;
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
    }
}
