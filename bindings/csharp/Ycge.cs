// bindings/csharp/Ycge.cs - P/Invoke declarations of include/ycge.h (libycge_hip.so, ABI 8).
//
// Drop into ConsoleGame/RayTracing/Native/.  Style follows the reference's own P/Invokes ([DllImport] + [StructLayout(LayoutKind.Sequential)]
// blittable structs, Renderer/Win32TerminalRenderer.cs:122-151).  Every structure is blittable (fixed buffers, no marshalled arrays), so `ref`
// passes the address of the managed value itself.
//
// MACHINE-CHECKED: tests/test_csharp_binding.py parses this file and holds every struct (field order, types, offsets, size) and every
// DllImport (name, parameter kinds, return kind) to yetanotherconsolegameengine_amd/abi.py, which tests/test_host_cpu.py holds to the
// header through the built library.  One declaration per line, one struct field list per `public` statement: keep it parseable.
using System;
using System.Runtime.InteropServices;

namespace ConsoleGame.RayTracing.Native
{
    [StructLayout(LayoutKind.Sequential)]
    public struct YVec3               // ycge_vec3
    {
        public float X, Y, Z;
        public YVec3(float x, float y, float z) { X = x; Y = y; Z = z; }
        public YVec3(ConsoleGame.RayTracing.Vec3 v) { X = v.X; Y = v.Y; Z = v.Z; }
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YMaterial           // ycge_material
    {
        public int Kind;              // YMaterialKind
        public YVec3 Albedo;
        public YVec3 AlbedoB;
        public float CheckerScale;
        public float Specular;
        public float Reflectivity;
        public YVec3 Emission;
        public float Transparency;
        public float IndexOfRefraction;
        public YVec3 TransmissionColor;
        public int Texture;           // index into YScene.Textures (Kind == Textured)
        public int Reserved;
        public double TextureWeight;  // Material.TextureWeight / UVScale as the doubles they are (Material.cs:17-18)
        public double UvScale;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YTexture            // ycge_texture
    {
        public int Width, Height;
        public IntPtr Pixels;         // static: Texture.pixels (int[] of RGBA32.ToInt()), pinned for the call
        public int FrameBytesPerPixel; // live (Texture(IFrameReader, useRGBA, flipU, flipV)): 3 = BGR, 4 = BGRA; 0 = static
        public int FlipU, FlipV;
        public IntPtr Frame;          // live: reader.GetCurrentFramePtr() at upload (may be null)
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct YPrim        // ycge_prim
    {
        public int Type;              // YPrimType
        public int Material;
        public int Ref;
        public int Reserved;
        public fixed float P[12];
        public float Specular;
        public float Reflectivity;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YMesh               // ycge_mesh
    {
        public IntPtr Triangles;      // 9 floats per triangle: A, B, C
        public int NTriangles;
        public int Material;
        public IntPtr TriMaterial;    // optional int per triangle
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YVoxelLookup        // ycge_voxel_lookup
    {
        public int MatId, MetaId, Material;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YGrid               // ycge_grid
    {
        public int Nx, Ny, Nz;
        public YVec3 MinCorner;
        public YVec3 VoxelSize;
        public IntPtr Cells;          // 2 ints per cell, (ix * ny + iy) * nz + iz
        public IntPtr Lookup;         // YVoxelLookup[]
        public int NLookup;
        public int DefaultMaterial;
        public int Wireframe;
        public float WireWidthFraction;
        public float WireMaxDistance;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YLight              // ycge_light
    {
        public YVec3 Position;
        public YVec3 Color;
        public float Intensity;
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YScene              // ycge_scene
    {
        public IntPtr Materials;
        public int NMaterials;
        public IntPtr Prims;
        public int NPrims;
        public IntPtr Meshes;
        public int NMeshes;
        public IntPtr Grids;
        public int NGrids;
        public IntPtr Lights;
        public int NLights;
        public YVec3 AmbientColor;
        public float AmbientIntensity;
        public YVec3 BackgroundTop;
        public YVec3 BackgroundBottom;
        public int IsVolumeScene;
        public int NTextures;
        public IntPtr Textures;
        public int HasDynamicTextures;
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct YConfig      // ycge_config - fill with ycge_config_default, then set the size
    {
        public int AbiVersion, FbWidth, FbHeight, SuperSample;
        public float FovDeg;
        public int Device, Rank, WorldSize;
        public int DiffuseBounces, MaxMirrorBounces, MaxRefractions;
        public float MirrorThreshold, Eps;
        public ulong SeedSalt;
        public float TaaAlpha, MotionTransReset, MotionRotReset, DiffuseSigmaDeg;
        public int TaaClampRadius;
        public float TaaLuminancePad;
        public int AtrousIterations;
        public float AtrousCPhi, AtrousNPhi, AtrousZPhi, AtrousAPhi;
        public int CaptureDebug, CountWork;
        public int SlabAlbedo;
        public int NDevices;
        public fixed int Devices[8];
        public int AtrousInplaceExact;
        public int TileRing;
        public int MultiDeviceExchange;   // YExchange: 0 = the peers push their tiles (default), 1 = RCCL all-gather inside ycge_render_frame
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct YFrameStats  // ycge_frame_stats
    {
        public long Frame;
        public int HistoryReset, FanBlocks;   // FanBlocks: reserved, always 0
        public double TraceMs, TaaMs, PostMs, TotalMs;
        public ulong NRays, NBox, NTri, NPrim, NVox;
        public float Exposure, ExposureSerialChunks;
        public ulong NRaysDark;
        public int NDevicesTraced;
        public fixed int DeviceTiles[8];
    }

    [StructLayout(LayoutKind.Sequential)]
    public struct YFlightInfo         // ycge_flight_info
    {
        public int TwoTraceStreams, PlacedGate, PostGate, PostPair, FramesOutstanding, StagePipeline;
        public ulong PlacedWaits;
    }

    // ycge_obj_info (an out parameter only, never embedded: C#'s default struct layout is the sequential one the C side has)
    public struct YObjInfo
    {
        public int NPositions, NTriangles;
        public long NLines;
        public int OnDevice, Reserved;
    }

    // ycge_voxel_edit, 36 bytes: every cell of the inclusive box Lo..Hi becomes (MatId, MetaId) (passed by address only, as above)
    public unsafe struct YVoxelEdit
    {
        public int GridIndex;         // resident grid; 0 for ycge_world_store_edit
        public fixed int Lo[3];
        public fixed int Hi[3];
        public int MatId, MetaId;
    }

    // ycge_camera_body, 40 bytes: what VolumeScene keeps between ticks (passed by address only, as above)
    public unsafe struct YCameraBody
    {
        public fixed float Pos[3];
        public float VerticalVelocity, ShiftHoldTimer;
        public fixed float RepelVel[3];
        public int AutoPlaced, IsGrounded;
    }

    // ycge_camera_world, 12 bytes: WorldConfig.WorldHeight, WaterLevel, VoxelSize.Y
    public struct YCameraWorld
    {
        public float WorldHeight, WaterLevel, VoxelSizeY;
    }

    // ycge_camera_move, 16 bytes: one HandleInput call's effect on the body (Kind: Ycge.CameraMove*; A, B: dx, dz or dy)
    public struct YCameraMove
    {
        public int Kind, Shift;
        public float A, B;
    }

    // ycge_camera_tick_info, 48 bytes (an out parameter only, as above)
    public struct YCameraTickInfo
    {
        public uint RaysCommitted, RaysWalked, Windows;
        public uint MicroSteps, BlockedSteps, Slides, PushOuts, EmbeddedResolutions, GroundSnaps, AutoPlacements, FailSafes;
        public uint Reserved;
    }

    // ycge_body_shape, 24 bytes: how big a body is and how it jumps and falls (VolumeScenes.cs:20-39 as data; ycge_volume_bodies_tick)
    public struct YBodyShape
    {
        public float EyeHeight, CollisionRadius, ProbeRadius, GroundClearance, JumpSpeed, GravityAccel;
        public static YBodyShape Default => new YBodyShape { EyeHeight = 1.7f, CollisionRadius = 0.65f, ProbeRadius = 0.35f, GroundClearance = 0.10f, JumpSpeed = 4.8f, GravityAccel = 9.81f };   // YCGE_BODY_SHAPE_DEFAULT
    }

    // ycge_body_result, 8 bytes: Status 0 committed, 1 / 2 a horizontal / vertical move reached the micro-step cap, 3 the position stopped being finite
    public struct YBodyResult
    {
        public int Status, BadMove;
    }

    // ycge_obj_ground_info, 64 bytes (an out parameter only, as above)
    public struct YObjGroundInfo
    {
        public float MinX, MinY, MinZ, MaxX, MaxY, MaxZ;
        public float CentroidX, CentroidY, CentroidZ;
        public float Extent;
        public int NComponents;
        public int ComponentFaces, ComponentVertices, FirstFace;
        public int OnDevice, Reserved;
    }

    // ycge_ansi_async, 48 bytes: the request of ycge_render_frame_async_ansi (passed by address only, as above)
    public struct YAnsiAsync
    {
        public int ConsoleW, ConsoleH, ViewportX, ViewportY, DefaultFg16, DefaultBg16, ClearScreen;
        public int Rgb;               // 0: 38;5 / 48;5 indices, 1: 24-bit triples
        public int Delta;             // 0: the full stream, 1: the delta stream
        public int MergeGap, Tolerance, Keyframe;   // delta only; Tolerance with Rgb only; otherwise 0
    }

    // ycge_ansi_async_result, 32 bytes: the record the device fills, in page-locked memory of the library (ycge_alloc_host_buffer)
    public unsafe struct YAnsiAsyncResult
    {
        public ulong Length;
        public fixed uint Info[4];    // {keyframe returned, changed, emitted, run starts}
        public uint Status, Reserved; // Status 1: the device stream exceeded the capacity, nothing was copied
    }

    public enum YStatus { Ok = 0, InvalidArg = -1, NoScene = -2, Device = -3, Unsupported = -4, OutOfMemory = -5, StackDepth = -6, NoDeviceCode = -7, Internal = -8 }
    public enum YMaterialKind { Constant = 0, Checker = 1, Textured = 2 }
    public enum YExchange { PeerPush = 0, Rccl = 1 }
    public enum YPrimType { Sphere = 0, Plane = 1, Disk = 2, XYRect = 3, XZRect = 4, YZRect = 5, Box = 6, CylinderY = 7, Triangle = 8, Mesh = 9, VolumeGrid = 10 }
    public enum YBuffer { Rays = 0, PrimId = 1, SubId = 2, HitT = 3, CurrentHdr = 4, GAlbedo = 5, GNormal = 6, GDepth = 7, SkyMask = 8, TaaHistory = 9, PrevNormal = 10, PrevDepth = 11, PrevSky = 12, Denoised = 13, RngState = 14 }
    public enum YAccel { SceneNodes = 0, SceneLeafIndex = 1, MeshNodes = 2, MeshLeafIndex = 3 }

    internal static unsafe class Ycge
    {
        public const int AbiVersion = 10;
        public const int MaxDevices = 8;
        public const int WorldStoreFields = 0;          // YCGE_WORLD_STORE_FIELDS: the window's 2-D fields stay resident
        public const int CameraMoveHorizontal = 0, CameraMoveVertical = 1, CameraMoveJump = 2, CameraMoveShift = 3;   // YCGE_CAMERA_MOVE_*
        public const int CameraMaxMoves = 32;           // YCGE_CAMERA_MAX_MOVES
        public const int BodiesMax = 4096;              // YCGE_BODIES_MAX
        public const int WorldStoreCells = 1;           // YCGE_WORLD_STORE_CELLS: the ordinary cell store, written on the device
        private const string Lib = "ycge_hip";       // libycge_hip.so

        [DllImport(Lib)] public static extern int ycge_config_default(ref YConfig cfg);
        [DllImport(Lib)] public static extern int ycge_create(ref YConfig cfg, out IntPtr ctx);
        [DllImport(Lib)] public static extern void ycge_destroy(IntPtr ctx);
        [DllImport(Lib)] public static extern IntPtr ycge_last_error(IntPtr ctx);
        [DllImport(Lib)] public static extern int ycge_scene_upload(IntPtr ctx, ref YScene scene);
        [DllImport(Lib)] public static extern int ycge_validate_scene(ref YScene scene, byte* msg, UIntPtr msgBytes);
        [DllImport(Lib)] public static extern int ycge_scene_update_lights(IntPtr ctx, YLight* lights, int nLights, YVec3* ambientColor, float ambientIntensity, YVec3* top, YVec3* bottom);
        [DllImport(Lib)] public static extern int ycge_scene_update_objects(IntPtr ctx, YPrim* prims, int nPrims);
        // chunk streaming (found by symbol lookup, ABI stays 10): grids beside those of the last upload, and their slots given back
        [DllImport(Lib)] public static extern int ycge_scene_attach_grids(IntPtr ctx, YGrid* grids, int n, int* outGridIndex);
        [DllImport(Lib)] public static extern int ycge_scene_detach_grids(IntPtr ctx, int* gridIndex, int n);
        // meshes and materials of a resident scene (found by symbol lookup, ABI stays 10): meshes beside those of the last upload and their indices
        // given back, materials behind the existing ones, the held OBJ as a resident mesh (translateOrTarget: 3 floats; outBounds: 6 floats or null)
        [DllImport(Lib)] public static extern int ycge_scene_attach_meshes(IntPtr ctx, YMesh* meshes, int n, int* outMeshIndex);
        [DllImport(Lib)] public static extern int ycge_scene_detach_meshes(IntPtr ctx, int* meshIndex, int n);
        [DllImport(Lib)] public static extern int ycge_scene_append_materials(IntPtr ctx, YMaterial* materials, int n, int* outFirstIndex);
        [DllImport(Lib)] public static extern int ycge_scene_attach_obj_mesh(IntPtr ctx, int autoGround, int normalize, float targetSize, float scale, float* translateOrTarget,
                                                                             int material, int* outMeshIndex, float* outBounds);
        // chunk generation (found by symbol lookup, ABI stays 10): WorldGenerator.GenerateChunkCells on the host / on the device + attach
        // (YWorld: bindings/csharp/YcgeWorld.cs)
        [DllImport(Lib)] public static extern int ycge_worldgen_chunk_cells(ref YWorld world, int cx, int cy, int cz, int* cellsOut, int* anySolidOut);
        [DllImport(Lib)] public static extern int ycge_scene_generate_grids(IntPtr ctx, ref YWorld world, int* keys, int n, YGrid* proto, int* outGridIndex, int* cellsOut);
        // the pregenerated world (WorldManager.GenerateAndSaveWorld) on the host / on the device + attach; HipPregenWorld in YcgeWorld.cs
        [DllImport(Lib)] public static extern int ycge_worldgen_world_cells(ref YWorld world, int chunksX, int chunksZ, int originBx, int originBz, int* cellsOut);
        [DllImport(Lib)] public static extern int ycge_scene_generate_world(IntPtr ctx, ref YWorld world, int chunksX, int chunksZ, int originBx, int originBz, YGrid* proto, int* outGridIndex, int* cellsOut);
        // the world store (found by symbol lookup, ABI stays 10): a VG01 payload resident on the device, its chunks attached by key; HipWorldStore in YcgeWorld.cs
        [DllImport(Lib)] public static extern int ycge_world_file_info(byte* bytes, UIntPtr nBytes, int* dimsOut, UIntPtr* payloadOffsetOut, byte* msg, UIntPtr msgBytes);
        [DllImport(Lib)] public static extern int ycge_world_store_load(IntPtr ctx, int* cells, int nx, int ny, int nz, int chunkSize);
        [DllImport(Lib)] public static extern int ycge_world_store_info(IntPtr ctx, int* dimsOut, int* chunkSizeOut, byte* occupiedOut, UIntPtr capacity);
        [DllImport(Lib)] public static extern int ycge_scene_attach_world_chunks(IntPtr ctx, int* keys, int n, YGrid* proto, int* outGridIndex);
        [DllImport(Lib)] public static extern int ycge_world_store_release(IntPtr ctx);
        // the store made by the generator on the device (form: WorldStoreFields / WorldStoreCells) and its x-planes read back, VG01 payload order
        [DllImport(Lib)] public static extern int ycge_world_store_generate(IntPtr ctx, ref YWorld world, int chunksX, int chunksZ, int originBx, int originBz, int form);
        [DllImport(Lib)] public static extern int ycge_world_store_read(IntPtr ctx, int x0, int planes, int* cellsOut);
        // voxel edits of resident grids and of the world store (found by symbol lookup, ABI stays 10); HipVoxelEdits in YcgeWorld.cs
        [DllImport(Lib)] public static extern int ycge_scene_edit_voxels(IntPtr ctx, YVoxelEdit* ops, int n, uint* outInfo);
        [DllImport(Lib)] public static extern int ycge_world_store_edit(IntPtr ctx, YVoxelEdit* ops, int n);
        // the pool of materialised chunks that lets a fields store take edits (found by symbol lookup, ABI stays 10); HipWorldStore.ReserveEdits in YcgeWorld.cs
        [DllImport(Lib)] public static extern int ycge_world_store_reserve_edits(IntPtr ctx, int maxChunks);
        [DllImport(Lib)] public static extern int ycge_world_store_edit_slots(IntPtr ctx, int* capacityOut, int* usedOut);
        [DllImport(Lib)] public static extern int ycge_world_store_revert_chunks(IntPtr ctx, int* keys, int n);
        [DllImport(Lib)] public static extern int ycge_scene_update_texture(IntPtr ctx, int textureIndex, IntPtr frame, UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_resize(IntPtr ctx, int fbWidth, int fbHeight, int superSample);
        [DllImport(Lib)] public static extern int ycge_set_camera(IntPtr ctx, float* pos, float yaw, float pitch, float fovDeg);
        [DllImport(Lib)] public static extern int ycge_render_frame(IntPtr ctx, float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_render_frame_async(IntPtr ctx);
        [DllImport(Lib)] public static extern int ycge_render_frame_async_sdr(IntPtr ctx, float* outTopBottomSdr);
        // device chexel colours (after ABI 10, found by symbol lookup - AbiVersion is unchanged): the presenters' bytes beside the SDR frame
        [DllImport(Lib)] public static extern int ycge_render_frame_chexels(IntPtr ctx, float* outTopBottomSdr, byte* outColor16, byte* outAnsi, byte* outRgba, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_render_frame_async_chexels(IntPtr ctx, float* outTopBottomSdr, byte* outColor16, byte* outAnsi, byte* outRgba);
        // the ANSI presenter's escape stream built on the device (after ABI 10, found by symbol lookup): ANSITerminalRenderer.Render()'s bytes
        [DllImport(Lib)] public static extern int ycge_ansi_stream_bound(int consoleW, int consoleH, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_render_frame_ansi(IntPtr ctx, int consoleW, int consoleH, int viewportX, int viewportY, int defaultFg16,
                                                                         int defaultBg16, int clearScreen, byte* outStream, UIntPtr capacity, UIntPtr* outLen,
                                                                         float* outTopBottomSdr, YFrameStats* stats);
        // Video mode (after ABI 10, found by symbol lookup): VideoRenderer.TryFlipAndBlit of the frame IFrameReader.GetCurrentFramePtr() shows
        [DllImport(Lib)] public static extern int ycge_video_blit(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, float* outTopBottomSdr, byte* outColor16,
                                                                  byte* outAnsi, byte* outRgba);
        [DllImport(Lib)] public static extern int ycge_video_blit_ansi(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int consoleW, int consoleH, int viewportX,
                                                                       int viewportY, int defaultFg16, int defaultBg16, int clearScreen, byte* outStream, UIntPtr capacity,
                                                                       UIntPtr* outLen, float* outTopBottomSdr);
        // the delta ANSI stream (after ABI 10, found by symbol lookup): only the cells that changed since the last stream of the context; a
        // keyframe is the full stream.  outInfo: 4 words {keyframe returned, changed cells, emitted cells, run starts} or null
        [DllImport(Lib)] public static extern int ycge_render_frame_ansi_delta(IntPtr ctx, int consoleW, int consoleH, int viewportX, int viewportY, int defaultFg16,
                                                                               int defaultBg16, int clearScreen, int mergeGap, int keyframe, byte* outStream,
                                                                               UIntPtr capacity, UIntPtr* outLen, uint* outInfo, float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_video_blit_ansi_delta(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int consoleW, int consoleH,
                                                                             int viewportX, int viewportY, int defaultFg16, int defaultBg16, int clearScreen, int mergeGap,
                                                                             int keyframe, byte* outStream, UIntPtr capacity, UIntPtr* outLen, uint* outInfo,
                                                                             float* outTopBottomSdr);
        // 24-bit colour ANSI streams (after ABI 10, found by symbol lookup): the five calls above on sRGB8 triples (ESC[38;2;R;G;Bm); the
        // delta forms take a tolerance 0..255 behind mergeGap and compare against what the terminal shows
        [DllImport(Lib)] public static extern int ycge_ansi_rgb_stream_bound(int consoleW, int consoleH, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_render_frame_ansi_rgb(IntPtr ctx, int consoleW, int consoleH, int viewportX, int viewportY, int defaultFg16,
                                                                             int defaultBg16, int clearScreen, byte* outStream, UIntPtr capacity, UIntPtr* outLen,
                                                                             float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_render_frame_ansi_rgb_delta(IntPtr ctx, int consoleW, int consoleH, int viewportX, int viewportY, int defaultFg16,
                                                                                   int defaultBg16, int clearScreen, int mergeGap, int tolerance, int keyframe,
                                                                                   byte* outStream, UIntPtr capacity, UIntPtr* outLen, uint* outInfo,
                                                                                   float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_video_blit_ansi_rgb(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int consoleW, int consoleH,
                                                                           int viewportX, int viewportY, int defaultFg16, int defaultBg16, int clearScreen, byte* outStream,
                                                                           UIntPtr capacity, UIntPtr* outLen, float* outTopBottomSdr);
        [DllImport(Lib)] public static extern int ycge_video_blit_ansi_rgb_delta(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int consoleW, int consoleH,
                                                                                 int viewportX, int viewportY, int defaultFg16, int defaultBg16, int clearScreen, int mergeGap,
                                                                                 int tolerance, int keyframe, byte* outStream, UIntPtr capacity, UIntPtr* outLen,
                                                                                 uint* outInfo, float* outTopBottomSdr);
        // quadrant-glyph frames (after ABI 10, found by symbol lookup): a chexel's 2 x 2 sub-cell colours (12 floats), the fitted glyph (UTF-16 code
        // units) and two colours (the RGBA plane, row 2 cy the foreground); the 24-bit streams with them.  superSample must be even; minContrast 0..255
        [DllImport(Lib)] public static extern int ycge_render_frame_quadrants(IntPtr ctx, float* outTopBottomSdr, float* outQuadSdr, ushort* outGlyphs, byte* outRgba,
                                                                              int minContrast, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_render_frame_ansi_quad(IntPtr ctx, int consoleW, int consoleH, int viewportX, int viewportY, int defaultFg16,
                                                                              int defaultBg16, int clearScreen, int minContrast, byte* outStream, UIntPtr capacity,
                                                                              UIntPtr* outLen, float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_render_frame_ansi_quad_delta(IntPtr ctx, int consoleW, int consoleH, int viewportX, int viewportY, int defaultFg16,
                                                                                    int defaultBg16, int clearScreen, int mergeGap, int tolerance, int keyframe,
                                                                                    int minContrast, byte* outStream, UIntPtr capacity, UIntPtr* outLen, uint* outInfo,
                                                                                    float* outTopBottomSdr, YFrameStats* stats);
        // ... and of a video frame: the video calls with minContrast where the frame forms have it; the SDR is ycge_video_blit's bit for bit
        [DllImport(Lib)] public static extern int ycge_video_blit_quadrants(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, float* outTopBottomSdr,
                                                                            float* outQuadSdr, ushort* outGlyphs, byte* outRgba, int minContrast);
        [DllImport(Lib)] public static extern int ycge_video_blit_ansi_quad(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int consoleW, int consoleH,
                                                                            int viewportX, int viewportY, int defaultFg16, int defaultBg16, int clearScreen, int minContrast,
                                                                            byte* outStream, UIntPtr capacity, UIntPtr* outLen, float* outTopBottomSdr);
        [DllImport(Lib)] public static extern int ycge_video_blit_ansi_quad_delta(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int consoleW, int consoleH,
                                                                                  int viewportX, int viewportY, int defaultFg16, int defaultBg16, int clearScreen, int mergeGap,
                                                                                  int tolerance, int keyframe, int minContrast, byte* outStream, UIntPtr capacity,
                                                                                  UIntPtr* outLen, uint* outInfo, float* outTopBottomSdr);
        // sixel frames (after ABI 10, found by symbol lookup): the picture is the hi-res buffer, fbW * superSample by 2 * fbH * superSample pixels.  The
        // planes (RGBA8 and the registers of the 6 x 6 x 6 cube, any of them null), the stream at a viewport cell, its bound, and the host encoder of a
        // register plane (no context); dither 0 or 1
        [DllImport(Lib)] public static extern int ycge_sixel_stream_bound(int pxW, int pxH, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_render_frame_pixels(IntPtr ctx, float* outTopBottomSdr, byte* outRgba, byte* outIndex, int dither, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_render_frame_sixel(IntPtr ctx, int viewportX, int viewportY, int clearScreen, int dither, byte* outStream,
                                                                          UIntPtr capacity, UIntPtr* outLen, float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_sixel_encode_host(byte* index, int pxW, int pxH, int viewportX, int viewportY, int clearScreen, byte* outStream,
                                                                         UIntPtr capacity, UIntPtr* outLen);
        // sixel in Video mode and the delta sixel streams (found by symbol lookup, ABI stays 10): the blit's hi-res samples as planes or as a stream, and the
        // streams that repaint only the bands and columns that changed against the last sixel stream handed out (outInfo: keyframe, bands, pixels, lines)
        [DllImport(Lib)] public static extern int ycge_video_blit_pixels(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, float* outTopBottomSdr, byte* outRgba,
                                                                         byte* outIndex, int dither);
        [DllImport(Lib)] public static extern int ycge_video_blit_sixel(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int viewportX, int viewportY,
                                                                        int clearScreen, int dither, byte* outStream, UIntPtr capacity, UIntPtr* outLen, float* outTopBottomSdr);
        [DllImport(Lib)] public static extern int ycge_render_frame_sixel_delta(IntPtr ctx, int viewportX, int viewportY, int clearScreen, int keyframe, int dither, byte* outStream,
                                                                                UIntPtr capacity, UIntPtr* outLen, uint* outInfo, float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_video_blit_sixel_delta(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int viewportX, int viewportY,
                                                                              int clearScreen, int keyframe, int dither, byte* outStream, UIntPtr capacity, UIntPtr* outLen,
                                                                              uint* outInfo, float* outTopBottomSdr);
        [DllImport(Lib)] public static extern int ycge_sixel_encode_delta_host(byte* prevIndex, byte* index, int pxW, int pxH, int viewportX, int viewportY, byte* outStream,
                                                                               UIntPtr capacity, UIntPtr* outLen, uint* outInfo);
        // the adaptive sixel palette (found by symbol lookup, ABI stays 10): up to 256 median-cut registers built on the device from the picture at hand
        // (hold 0) or kept from the last build (hold 1); outPalette 256 x RGBA8 and outCount may be null; the rule and the stream in plain C (no context)
        [DllImport(Lib)] public static extern int ycge_sixel_palette_stream_bound(int pxW, int pxH, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_render_frame_sixel_palette(IntPtr ctx, int viewportX, int viewportY, int clearScreen, int hold, byte* outStream,
                                                                                  UIntPtr capacity, UIntPtr* outLen, byte* outPalette, int* outCount, float* outTopBottomSdr,
                                                                                  YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_video_blit_sixel_palette(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, int viewportX, int viewportY,
                                                                                int clearScreen, int hold, byte* outStream, UIntPtr capacity, UIntPtr* outLen, byte* outPalette,
                                                                                int* outCount, float* outTopBottomSdr);
        [DllImport(Lib)] public static extern int ycge_render_frame_pixels_palette(IntPtr ctx, float* outTopBottomSdr, byte* outRgba, byte* outIndex, int hold, byte* outPalette,
                                                                                   int* outCount, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_video_blit_pixels_palette(IntPtr ctx, IntPtr frame, int srcW, int srcH, int bytesPerPixel, float* outTopBottomSdr,
                                                                                 byte* outRgba, byte* outIndex, int hold, byte* outPalette, int* outCount);
        [DllImport(Lib)] public static extern int ycge_sixel_palette_host(byte* rgba, int pxW, int pxH, byte* outIndex, byte* outPalette, byte* outPct, int* outCount);
        [DllImport(Lib)] public static extern int ycge_sixel_encode_palette_host(byte* index, byte* pct, int count, int pxW, int pxH, int viewportX, int viewportY, int clearScreen,
                                                                                 byte* outStream, UIntPtr capacity, UIntPtr* outLen);
        // the console's other framebuffers for every stream call above (found by symbol lookup, ABI stays 10); YConsoleLayer, YChexel and
        // HipConsoleLayers: bindings/csharp/YcgeConsole.cs
        [DllImport(Lib)] public static extern int ycge_console_set_layers(IntPtr ctx, YConsoleLayer* layers, int n, int raytraceAt);
        // the four frame forms of the streams with frames in flight (found by symbol lookup, ABI stays 10): outStream (16-byte aligned) and outResult
        // in page-locked memory, both the caller's to read after ycge_wait
        [DllImport(Lib)] public static extern int ycge_render_frame_async_ansi(IntPtr ctx, YAnsiAsync* req, byte* outStream, UIntPtr capacity, YAnsiAsyncResult* outResult,
                                                                               float* outTopBottomSdr);
        // OBJ meshes from file bytes (MeshLoader.FromObj on the device; HipObjLoader.cs).  info: a YObjInfo
        [DllImport(Lib)] public static extern int ycge_obj_parse_host(byte* text, UIntPtr bytes, float* positions, int* faces, out YObjInfo info, byte* msg, UIntPtr msgBytes);
        [DllImport(Lib)] public static extern int ycge_obj_parse(IntPtr ctx, byte* text, UIntPtr bytes, out YObjInfo info);
        [DllImport(Lib)] public static extern int ycge_obj_read(IntPtr ctx, float* positions, int* faces);
        [DllImport(Lib)] public static extern int ycge_obj_triangles(IntPtr ctx, int normalize, float targetSize, float scale, float* translate, float* outTriangles, float* outBounds);
        [DllImport(Lib)] public static extern int ycge_obj_release(IntPtr ctx);
        // MeshScenes.AddMeshAutoGround on the held OBJ (largest component, centroid, bounds on the device).  info: a YObjGroundInfo; outInfo may be null
        [DllImport(Lib)] public static extern int ycge_obj_ground_host(float* positions, int nPositions, int* faces, int nTriangles, out YObjGroundInfo info);
        [DllImport(Lib)] public static extern int ycge_obj_ground(IntPtr ctx, out YObjGroundInfo info);
        [DllImport(Lib)] public static extern int ycge_obj_triangles_auto_ground(IntPtr ctx, float scale, float* target, float* outTriangles, float* outBounds, YObjGroundInfo* outInfo);
        [DllImport(Lib)] public static extern int ycge_wait(IntPtr ctx);
        [DllImport(Lib)] public static extern int ycge_async_trace_times(IntPtr ctx, float* msOut, int capacity, out int nOut);
        [DllImport(Lib)] public static extern int ycge_flight_query(IntPtr ctx, out YFlightInfo info);
        [DllImport(Lib)] public static extern int ycge_exchange_query(IntPtr ctx, out int mode, out int world);
        // one process per GPU (INTEGRATION.md section 5): device pointers and HIP streams travel as IntPtr
        [DllImport(Lib)] public static extern int ycge_tile_slab_bytes(IntPtr ctx, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_trace_tiles(IntPtr ctx, IntPtr dSlab, IntPtr stream, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_resolve_gathered(IntPtr ctx, IntPtr dAllSlabs, IntPtr stream, float* outTopBottomSdr, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_halo_counts(IntPtr ctx, long* sendCounts, long* recvCounts);
        [DllImport(Lib)] public static extern int ycge_history_slab_bytes(IntPtr ctx, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_trace_tiles_resident(IntPtr ctx, IntPtr dHaloSend, IntPtr stream, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_trace_tiles_resident_batch(IntPtr ctx, int n, float* poses, IntPtr* dHaloSends, IntPtr stream);
        [DllImport(Lib)] public static extern int ycge_resolve_tiles_resident(IntPtr ctx, IntPtr dHaloRecv, IntPtr dHistorySlab, IntPtr stream, YFrameStats* stats);
        [DllImport(Lib)] public static extern int ycge_unpack_history(IntPtr ctx, IntPtr dAllHistorySlabs, IntPtr stream);
        // tests / tools
        // scene queries (ABI 10): Scene.Hit / Scene.Occluded for a batch of rays, beside a frame in flight (HipSceneQuery.cs)
        [DllImport(Lib)] public static extern int ycge_scene_hit(IntPtr ctx, float[] rays, int n, float[] hits, int[] ids);
        [DllImport(Lib)] public static extern int ycge_scene_occluded(IntPtr ctx, float[] rays, int n, byte[] occluded);
        // VolumeScene's camera physics, one launch a tick (found by symbol lookup, ABI stays 10); HipVolumeCamera.cs
        [DllImport(Lib)] public static extern int ycge_volume_camera_tick(IntPtr ctx, YCameraBody* body, YCameraWorld* world, YCameraMove* moves, int nMoves,
                                                                          float deltaTimeMs, int runUpdate, YCameraTickInfo* info);
        // many bodies a tick in one launch, each with its own shape (found by symbol lookup, ABI stays 10); HipVolumeBodies.cs
        [DllImport(Lib)] public static extern int ycge_volume_bodies_tick(IntPtr ctx, YCameraBody* bodies, YBodyShape* shapes, int n, YCameraWorld* world, YCameraMove* moves,
                                                                          int* moveFirst, float deltaTimeMs, int runUpdate, YBodyResult* results, YCameraTickInfo* info);
        [DllImport(Lib)] public static extern int ycge_read_buffer(IntPtr ctx, int which, IntPtr dst, UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_set_frame_counter(IntPtr ctx, long frameCounter);
        [DllImport(Lib)] public static extern int ycge_read_timed_steps(IntPtr ctx, out ulong laneSteps);
        [DllImport(Lib)] public static extern int ycge_device_count();
        // page-locked memory for the SDR frame (ABI 8): the library's own, or whole pages the caller owns
        [DllImport(Lib)] public static extern UIntPtr ycge_host_page_size();
        [DllImport(Lib)] public static extern int ycge_alloc_host_buffer(UIntPtr bytes, out IntPtr buffer);
        [DllImport(Lib)] public static extern int ycge_free_host_buffer(IntPtr buffer);
        [DllImport(Lib)] public static extern int ycge_pin_host_buffer(IntPtr buffer, UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_unpin_host_buffer(IntPtr buffer);
        [DllImport(Lib)] public static extern int ycge_accel_size(IntPtr ctx, int which, int index, out UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_read_accel(IntPtr ctx, int which, int index, IntPtr dst, UIntPtr bytes);
        [DllImport(Lib)] public static extern int ycge_device_info(IntPtr ctx, byte* name, UIntPtr nameBytes, out int computeUnits);

        /// <summary>Status codes back into the exceptions the reference throws on misuse (e.g. Scenes/Scene.cs:73).</summary>
        public static void Check(IntPtr ctx, int rc)
        {
            if (rc == 0) return;
            string msg = Marshal.PtrToStringAnsi(ycge_last_error(ctx)) ?? "";
            switch ((YStatus)rc)
            {
                case YStatus.NoScene: throw new InvalidOperationException(msg);
                case YStatus.InvalidArg: throw new ArgumentException(msg);
                case YStatus.Unsupported: throw new NotSupportedException(msg);
                case YStatus.OutOfMemory: throw new OutOfMemoryException(msg);
                case YStatus.Internal: throw new InvalidOperationException("ycge internal error (a C++ exception was stopped at the C-ABI): " + msg);
                default: throw new Exception("ycge " + ((YStatus)rc) + ": " + msg);
            }
        }
    }
}
