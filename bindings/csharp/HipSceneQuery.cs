// bindings/csharp/HipSceneQuery.cs - Scene.Hit / Scene.Occluded (Scenes/Scene.cs:71-82) answered on the device scene of a HipRaytraceWrapper
// (ycge_scene_hit / ycge_scene_occluded, ABI 10).
//
// The reference's other caller of Scene.Hit is VolumeScene's camera physics (ground fan, collision capsule, push-out: Scenes/VolumeScenes.cs),
// which runs in Update between two TryFlipAndBlit calls.  With the wrapper the scene lives on the GPU, rebuilt there by
// ycge_scene_update_objects as WorldManager streams chunks; these calls ask that copy instead of a second CPU-side BVH.  A query sees the
// scene as the wrapper's last SyncScene left it (the objects of the last TryFlipAndBlit), and runs beside a FrameLate frame in flight
// without waiting for it.  INTEGRATION.md section 6.
//
// Records: T, P and N as the reference's HitRecord has them (U = V = 0 - the probes never read them); the material's albedo and the
// Scene.Objects index of the hit travel beside the record (Material itself is a delegate's output the device does not keep).
// The library normalises the direction it is given as `new Ray(o, d)` does.  Hit(Vec3, Vec3, ...) passes the direction the caller would
// have handed to `new Ray` - the reference's query exactly; Hit(Ray, ...) passes r.Dir, which is normalised once more (the same ray up to
// the last bit of the direction).
using System;
using ConsoleGame.RayTracing;

namespace ConsoleGame.RayTracing.Native
{
    public sealed class HipSceneQuery
    {
        private readonly Func<IntPtr> context;
        private readonly float[] one = new float[8];
        private readonly float[] oneHit = new float[10];
        private readonly int[] oneId = new int[2];
        private readonly byte[] oneFlag = new byte[1];

        internal HipSceneQuery(Func<IntPtr> context) { this.context = context ?? throw new ArgumentNullException(nameof(context)); }

        /// <summary>Scene.Objects index of the last hit Hit reported (-1 after a miss).</summary>
        public int LastObject { get; private set; } = -1;
        /// <summary>Mat.Albedo of the last hit Hit reported.</summary>
        public Vec3 LastAlbedo { get; private set; }

        /// <summary>Scene.Hit(r, tMin, tMax, ref rec, 0, 0): fills rec.T, rec.P, rec.N (U = V = 0; rec.Mat is left as it was).</summary>
        public bool Hit(Ray r, float tMin, float tMax, ref HitRecord rec) => Hit(r.Origin, r.Dir, tMin, tMax, ref rec);

        /// <summary>Scene.Hit(new Ray(origin, dir), tMin, tMax, ref rec, 0, 0).</summary>
        public bool Hit(Vec3 origin, Vec3 dir, float tMin, float tMax, ref HitRecord rec)
        {
            Pack(one, 0, origin, dir, tMin, tMax);
            IntPtr ctx = context();
            Ycge.Check(ctx, Ycge.ycge_scene_hit(ctx, one, 1, oneHit, oneId));
            LastObject = oneId[0];
            if (oneId[0] < 0) { LastAlbedo = new Vec3(0f, 0f, 0f); return false; }
            rec.T = oneHit[0];
            rec.P = new Vec3(oneHit[1], oneHit[2], oneHit[3]);
            rec.N = new Vec3(oneHit[4], oneHit[5], oneHit[6]);
            rec.U = 0; rec.V = 0;
            LastAlbedo = new Vec3(oneHit[7], oneHit[8], oneHit[9]);
            return true;
        }

        /// <summary>Scene.Occluded(r, maxDist, 0, 0): anything in [0.001, maxDist] along r.</summary>
        public bool Occluded(Ray r, float maxDist)
        {
            Pack(one, 0, r.Origin, r.Dir, 0.001f, maxDist);
            IntPtr ctx = context();
            Ycge.Check(ctx, Ycge.ycge_scene_occluded(ctx, one, 1, oneFlag));
            return oneFlag[0] != 0;
        }

        /// <summary>Batched Scene.Hit: rays = n x {ox, oy, oz, dx, dy, dz, tMin, tMax}; hits = n x {t, p xyz, n xyz, albedo rgb};
        /// ids = n x {Scene.Objects index, sub} ({-1, -1} and a zero record on a miss).  One call for the five rays of the ground fan.</summary>
        public void HitBatch(float[] rays, int n, float[] hits, int[] ids)
        {
            if (rays == null || hits == null || ids == null) throw new ArgumentNullException(rays == null ? nameof(rays) : hits == null ? nameof(hits) : nameof(ids));
            if (n < 0 || rays.Length < 8L * n || hits.Length < 10L * n || ids.Length < 2L * n) throw new ArgumentException("arrays shorter than n rays");
            IntPtr ctx = context();
            Ycge.Check(ctx, Ycge.ycge_scene_hit(ctx, rays, n, hits, ids));
        }

        /// <summary>Batched Scene.Occluded / boolean of Scene.Hit: occluded[i] = 1 when ray i hits something in [tMin, tMax].</summary>
        public void OccludedBatch(float[] rays, int n, byte[] occluded)
        {
            if (rays == null || occluded == null) throw new ArgumentNullException(rays == null ? nameof(rays) : nameof(occluded));
            if (n < 0 || rays.Length < 8L * n || occluded.Length < n) throw new ArgumentException("arrays shorter than n rays");
            IntPtr ctx = context();
            Ycge.Check(ctx, Ycge.ycge_scene_occluded(ctx, rays, n, occluded));
        }

        /// <summary>Writes ray i of a batch: origin, direction (as given to `new Ray`), tMin, tMax.</summary>
        public static void Pack(float[] rays, int i, Vec3 origin, Vec3 dir, float tMin, float tMax)
        {
            int k = 8 * i;
            rays[k] = origin.X; rays[k + 1] = origin.Y; rays[k + 2] = origin.Z;
            rays[k + 3] = dir.X; rays[k + 4] = dir.Y; rays[k + 5] = dir.Z;
            rays[k + 6] = tMin; rays[k + 7] = tMax;
        }
    }
}
