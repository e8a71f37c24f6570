// bindings/csharp/HipVolumeBodies.cs - many bodies of a voxel world a tick, each with its own shape, on the device scene of a
// HipRaytraceWrapper: ycge_volume_bodies_tick, one launch for all of them.
//
// HipVolumeCamera moves one body of the reference's size a call.  A host that also moves mobs, dropped items, projectiles or the other players
// of a replicated scene (SyncScene.cs) keeps them here: Add() makes a body with its shape (YBodyShape.Default: the reference's 1.7-tall capsule
// of radius 0.65), Horizontal / Vertical / Jump / Shift queue what a HandleInput call would do to it, and Update() hands every body, its shape
// and its moves to the library once.  Each body comes back as VolumeScene's Update would have left it alone, bit for bit; a body whose move
// reached the library's micro-step cap stays as it was and says so in Results, the others commit.  INTEGRATION.md section 6.2.
using System;
using System.Collections.Generic;
using ConsoleGame.RayTracing;

namespace ConsoleGame.RayTracing.Native
{
    public sealed unsafe class HipVolumeBodies
    {
        private readonly Func<IntPtr> context;
        private readonly List<List<YCameraMove>> moves = new List<List<YCameraMove>>();
        private YCameraBody[] bodies = new YCameraBody[0];
        private YBodyShape[] shapes = new YBodyShape[0];
        private YBodyResult[] results = new YBodyResult[0];
        private YCameraTickInfo[] infos = new YCameraTickInfo[0];
        private YCameraWorld world;

        internal HipVolumeBodies(Func<IntPtr> context, float worldHeight, float waterLevel, float voxelSizeY)
        {
            this.context = context ?? throw new ArgumentNullException(nameof(context));
            world.WorldHeight = worldHeight; world.WaterLevel = waterLevel; world.VoxelSizeY = voxelSizeY;
        }

        public int Count { get; private set; }

        /// <summary>A new body; returns its index.  At most Ycge.BodiesMax bodies.</summary>
        public int Add(Vec3 pos, YBodyShape shape, bool autoPlaced = false)
        {
            if (Count == Ycge.BodiesMax) throw new InvalidOperationException("HipVolumeBodies holds at most Ycge.BodiesMax bodies");
            if (Count == bodies.Length)
            {
                int cap = Math.Max(16, 2 * Count);
                Array.Resize(ref bodies, cap); Array.Resize(ref shapes, cap); Array.Resize(ref results, cap); Array.Resize(ref infos, cap);
            }
            int i = Count++;
            bodies[i] = default;
            fixed (YCameraBody* b = &bodies[i]) { b->Pos[0] = pos.X; b->Pos[1] = pos.Y; b->Pos[2] = pos.Z; }
            bodies[i].AutoPlaced = autoPlaced ? 1 : 0;
            shapes[i] = shape;
            moves.Add(new List<YCameraMove>());
            return i;
        }
        public int Add(Vec3 pos, bool autoPlaced = false) => Add(pos, YBodyShape.Default, autoPlaced);

        public Vec3 Position(int i) { fixed (YCameraBody* b = &bodies[Checked(i)]) return new Vec3(b->Pos[0], b->Pos[1], b->Pos[2]); }
        public bool IsGrounded(int i) => bodies[Checked(i)].IsGrounded != 0;
        /// <summary>Status 0: the last Update committed body i; 1 / 2: a horizontal / vertical move reached the cap, 3: its position stopped being finite - the body is as it was.</summary>
        public YBodyResult Result(int i) => results[Checked(i)];
        public YCameraTickInfo Info(int i) => infos[Checked(i)];

        public void Horizontal(int i, Vec3 delta) => Queue(i, Ycge.CameraMoveHorizontal, 0, delta.X, delta.Z);
        public void Vertical(int i, float dy) => Queue(i, Ycge.CameraMoveVertical, 0, dy, 0.0f);
        public void Jump(int i, bool shiftDown = false) => Queue(i, Ycge.CameraMoveJump, shiftDown ? 1 : 0, 0.0f, 0.0f);
        public void Shift(int i) => Queue(i, Ycge.CameraMoveShift, 0, 0.0f, 0.0f);

        /// <summary>Every body's moves since the last call, then Update's physics with deltaTimeMS, in one launch.  Returns how many bodies committed.</summary>
        public int Update(float deltaTimeMS, bool runUpdate = true)
        {
            int n = Count;
            if (n == 0) return 0;
            var first = new int[n + 1];
            for (int i = 0; i < n; i++) first[i + 1] = first[i] + moves[i].Count;
            var flat = new YCameraMove[Math.Max(1, first[n])];
            for (int i = 0; i < n; i++) moves[i].CopyTo(flat, first[i]);
            IntPtr ctx = context();
            fixed (YCameraBody* b = bodies)
            fixed (YBodyShape* s = shapes)
            fixed (YCameraWorld* w = &world)
            fixed (YCameraMove* m = flat)
            fixed (int* f = first)
            fixed (YBodyResult* r = results)
            fixed (YCameraTickInfo* info = infos)
                Ycge.Check(ctx, Ycge.ycge_volume_bodies_tick(ctx, b, s, n, w, first[n] > 0 ? m : null, f, deltaTimeMS, runUpdate ? 1 : 0, r, info));
            int committed = 0;
            for (int i = 0; i < n; i++) { moves[i].Clear(); if (results[i].Status == 0) committed++; }
            return committed;
        }

        private void Queue(int i, int kind, int shift, float a, float b)
        {
            var list = moves[Checked(i)];
            if (list.Count == Ycge.CameraMaxMoves) throw new InvalidOperationException("a body takes at most Ycge.CameraMaxMoves moves a tick");
            list.Add(new YCameraMove { Kind = kind, Shift = shift, A = a, B = b });
        }
        private int Checked(int i) => (uint)i < (uint)Count ? i : throw new ArgumentOutOfRangeException(nameof(i));
    }
}
