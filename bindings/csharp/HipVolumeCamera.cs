// bindings/csharp/HipVolumeCamera.cs - VolumeScene's camera physics (Scenes/VolumeScenes.cs:51-159 Update, :165-213 HandleInput) on the device
// scene of a HipRaytraceWrapper: ycge_volume_camera_tick, one launch a tick.
//
// Through HipSceneQuery every Scene.Hit of the physics is a round trip to the GPU, and most of them depend on the one before.  This class
// keeps the fields VolumeScene keeps between ticks - CameraPos, verticalVelocity, shiftHoldTimer, repelVel, autoPlaced, isGrounded - as the
// library's ycge_camera_body, records what each HandleInput call would do to them as a move, and hands body and moves to the library once
// per Update.  The body that comes back is the one the reference's Update would have left, bit for bit.  LoadChunksAround, base.Update and
// the camera rotation stay in VolumeScene.  INTEGRATION.md section 6.
using System;
using System.Collections.Generic;
using ConsoleGame.RayTracing;

namespace ConsoleGame.RayTracing.Native
{
    public sealed unsafe class HipVolumeCamera
    {
        private const float ShiftSpeedMult = 30.0f;       // VolumeScenes.cs:32
        private readonly Func<IntPtr> context;
        private readonly List<YCameraMove> moves = new List<YCameraMove>();
        private YCameraBody body;
        private YCameraWorld world;

        internal HipVolumeCamera(Func<IntPtr> context, Vec3 cameraPos, float worldHeight, float waterLevel, float voxelSizeY, bool autoPlaced)
        {
            this.context = context ?? throw new ArgumentNullException(nameof(context));
            CameraPos = cameraPos;
            body.AutoPlaced = autoPlaced ? 1 : 0;
            world.WorldHeight = worldHeight; world.WaterLevel = waterLevel; world.VoxelSizeY = voxelSizeY;
        }

        public Vec3 CameraPos
        {
            get { fixed (YCameraBody* b = &body) return new Vec3(b->Pos[0], b->Pos[1], b->Pos[2]); }
            set { fixed (YCameraBody* b = &body) { b->Pos[0] = value.X; b->Pos[1] = value.Y; b->Pos[2] = value.Z; } }
        }
        public bool IsGrounded => body.IsGrounded != 0;
        public bool AutoPlaced => body.AutoPlaced != 0;
        public float VerticalVelocity => body.VerticalVelocity;
        /// <summary>What the last Update did: rays of the serial order, rays walked, windows, and the event counters.</summary>
        public YCameraTickInfo LastInfo { get; private set; }

        /// <summary>HandleInput's effect on the body for one key (:165-213).  Rotation keys are the caller's; yaw is the scene's Yaw after them.</summary>
        public void HandleInput(ConsoleKeyInfo keyInfo, float dt, float yaw)
        {
            if (dt < 0.0f) dt = 0.0f;
            float moveSpeed = 6.0f;
            bool shiftDown = (keyInfo.Modifiers & ConsoleModifiers.Shift) != 0;
            if (shiftDown)
            {
                moveSpeed *= ShiftSpeedMult;
                Add(Ycge.CameraMoveShift, 0, 0.0f, 0.0f);
            }
            float cy = MathF.Cos(yaw), sy = MathF.Sin(yaw);
            Vec3 forwardXZ = new Vec3(sy, 0.0, -cy);
            Vec3 rightXZ = new Vec3(cy, 0.0, sy);
            float k = moveSpeed * dt;
            switch (keyInfo.Key)
            {
                case ConsoleKey.W: Horizontal(forwardXZ * k); break;
                case ConsoleKey.S: Horizontal(-forwardXZ * k); break;
                case ConsoleKey.A: Horizontal(-rightXZ * k); break;
                case ConsoleKey.D: Horizontal(rightXZ * k); break;
                case ConsoleKey.E: Add(Ycge.CameraMoveVertical, 0, k, 0.0f); break;
                case ConsoleKey.Q: Add(Ycge.CameraMoveVertical, 0, -k, 0.0f); break;
                case ConsoleKey.Spacebar: Add(Ycge.CameraMoveJump, shiftDown ? 1 : 0, 0.0f, 0.0f); break;
            }
        }

        /// <summary>The moves since the last call, then Update's physics with deltaTimeMS, on the device; returns the new CameraPos.</summary>
        public Vec3 Update(float deltaTimeMS, bool runUpdate = true)
        {
            IntPtr ctx = context();
            YCameraTickInfo info = default;
            int done = 0;
            // the library takes at most Ycge.CameraMaxMoves moves a call: a burst of key events goes in several calls, the update with the last
            do
            {
                int n = Math.Min(moves.Count - done, Ycge.CameraMaxMoves);
                bool last = done + n == moves.Count;
                YCameraMove* batch = stackalloc YCameraMove[Math.Max(1, n)];
                for (int i = 0; i < n; i++) batch[i] = moves[done + i];
                fixed (YCameraBody* b = &body)
                fixed (YCameraWorld* w = &world)
                    Ycge.Check(ctx, Ycge.ycge_volume_camera_tick(ctx, b, w, n > 0 ? batch : null, n, deltaTimeMS, last && runUpdate ? 1 : 0, &info));
                done += n;
            } while (done < moves.Count);
            moves.Clear();
            LastInfo = info;
            return CameraPos;
        }

        private void Horizontal(Vec3 delta) => Add(Ycge.CameraMoveHorizontal, 0, delta.X, delta.Z);
        private void Add(int kind, int shift, float a, float b) => moves.Add(new YCameraMove { Kind = kind, Shift = shift, A = a, B = b });
    }
}
