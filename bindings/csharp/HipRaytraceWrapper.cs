// bindings/csharp/HipRaytraceWrapper.cs - the third IConsoleRenderer (next to RaytraceWrapper / VideoWrapper, RaytraceEntity.cs:20-50).
//
// RaytraceEntity is a `partial class` and its IConsoleRenderer is private: this file adds the wrapper as one more part of the class, so
// no existing file changes.  A construction site then reads
//     this.renderer = new HipRaytraceWrapper(fb, activeScene, activeScene.DefaultFovDeg, rtSuperSample);
// where it reads `new RaytraceWrapper(new RaytraceRenderer(fb, activeScene, fov, rtWidth, rtHeight, rtSuperSample))` today
// (RaytraceEntity.cs:97-98, 240-241, 262-263).
//
// One TryFlipAndBlit = one ycge_render_frame: ray generation, trace, TAA, denoise, exposure, tonemap and downsample on the GPU
// (RaytraceRenderer.cs:157-267), then the SetChexel loop of :260-261 on the host, unchanged.
//
// Options (HipRaytraceOptions, all off by default = the reference's behaviour call for call):
//   FrameLate  - TryFlipAndBlit queues frame N with ycge_render_frame_async_sdr and blits frame N - 1, which it waited for first: the GPU's
//                3.6 ms (trace + TAA + the exact post stage at 1080p) run beside the host's Update / input / presenter instead of in front
//                of them.  One frame of latency; the frames themselves are the same, in the same order (tests/test_gpu_timed_variants.py).
//   Devices    - one process, several GPUs: the ONE call drives them all (config.n_devices / devices[]).
//   Exchange   - how their tiles come together on Devices[0]: YExchange.PeerPush (xGMI peer writes) or YExchange.Rccl (ONE ncclAllGather of
//                the tile slabs inside ycge_render_frame - SURVEY 8(e); the library dlopens librccl.so and falls back to PeerPush without it;
//                ExchangeInUse says which).
//   DeviceChexelColors - the nearest-of-16 palette search of ChexelColor(Vec3) (Chexel.cs:70-89) runs on the GPU beside the tonemap
//                (ycge_render_frame_chexels / ycge_render_frame_async_chexels with FrameLate): the frame reads back the SDR array and one
//                byte a chexel {color_16 of top | of bottom << 4}, and the blit builds each ChexelColor from its byte and its Vec3 - every
//                field equals the reference's, the host no longer searches.  Needs a library that exports the two calls (INTEGRATION.md
//                section 7).
//   DeviceAnsiStream - with AnsiPresenter (a DeviceAnsiTerminalRenderer in place of ANSITerminalRenderer): the frame is read back as the
//                bytes ANSITerminalRenderer.Render() would write for the console (ycge_render_frame_ansi), and the presenter writes them to
//                stdout as they are - the framebuffer is not written and no cell is walked on the host.  With FrameLate the frame is queued
//                (ycge_render_frame_async_ansi, all four colour / delta combinations): two page-locked stream buffers and records rotate, the
//                device copies the exact length into one while the presenter writes the other, one frame late.  The presenter's other framebuffers - Terminal's entity framebuffer, a menu, a text entity - are composed on the
//                device as GetChexelForPoint composes them (ycge_console_set_layers, sent before every frame; INTEGRATION.md section 8).
//   DeviceAnsiDelta - with DeviceAnsiStream: a frame's bytes are the delta stream (ycge_render_frame_ansi_delta) - only the cells whose
//                ANSI pair changed since the last frame written, each run behind a cursor move, and always the console's last cell, so the
//                cursor ends where Render() leaves it for Terminal.Start's HUD.  The first frame, a frame after a console resize
//                (ClearPending) and a frame after a switch of geometry are keyframes: the full stream.  AnsiMergeGap: unchanged cells between
//                two changed ones of a row that are rewritten rather than jumped over (0..8).
//   AnsiTrueColor - with DeviceAnsiStream: the streams carry 24-bit colour (ycge_render_frame_ansi_rgb / _rgb_delta): ESC[38;2;R;G;Bm of the
//                sRGB8 triples OpenGLTerminalRenderer shows, not the 240 colours of ChexelToAnsi256.  With DeviceAnsiDelta a cell is rewritten
//                when a channel is more than AnsiRgbTolerance (0..255) away from what the terminal shows for it; 0 is the exact form.  The
//                library keeps one terminal state per context: a switch of colour form is a keyframe (INTEGRATION.md section 8.2).
//   QuadrantGlyphs - with DeviceAnsiStream: quadrant block glyphs (ycge_render_frame_ansi_quad / _quad_delta): each cell shows a 2 x 2 grid of
//                sub-cells in two 24-bit colours, fitted on the device - twice the horizontal detail in the same console.  superSample must
//                be even; the streams are synchronous (FrameLate is not offered with it) and 24-bit whatever AnsiTrueColor says.  With
//                DeviceAnsiDelta a cell is rewritten when its glyph differs or a channel is more than AnsiRgbTolerance away;
//                QuadrantMinContrast (0..255) keeps a cell one colour while its sub-cells lie that close to their mean, so that TAA's +-1
//                flicker does not flip glyphs in a resting picture (INTEGRATION.md section 8.5).
//   SixelGraphics - with DeviceAnsiStream: the frame's bytes are a DEC sixel stream (ycge_render_frame_sixel) of every hi-res sample the frame
//                traced - fbW * superSample by 2 * fbH * superSample pixels in the 216 colours of a 6 x 6 x 6 cube, SixelDither an ordered
//                4 x 4 dither - with its top left corner at the framebuffer's viewport cell.  Any superSample; synchronous (no FrameLate),
//                and the other framebuffers are not composed into the picture: the host writes its text cells behind the image.
//                The stream buffer is pageable memory of the bound's size (INTEGRATION.md section 8.6).  SixelDelta: the delta form
//                (ycge_render_frame_sixel_delta) - after the first picture a frame repaints only the bands and columns whose registers
//                changed, on the delta state the context shares with Video mode (HipVideoWrapper) and the ANSI delta calls.
//                SixelAdaptivePalette: up to 256 median-cut registers built on the device from the picture (ycge_render_frame_sixel_palette)
//                in place of the cube - no dither, no delta form; SixelHoldPalette keeps the palette of the first frame (hold = 1) so that
//                a picture at rest does not shimmer, and SixelRebuildPalette() asks the next frame for a new one.
using System;
using System.Collections.Generic;
using System.IO;
using System.Runtime.CompilerServices;
using ConsoleGame.RayTracing;
using ConsoleGame.RayTracing.Native;
using ConsoleGame.RayTracing.Objects;
using ConsoleGame.RayTracing.Scenes;
using ConsoleGame.Renderer;

public sealed class HipRaytraceOptions
{
    public bool FrameLate;
    public int[] Devices;
    public YExchange Exchange = YExchange.PeerPush;
    public bool DeviceChexelColors;
    public bool DeviceAnsiStream;
    public DeviceAnsiTerminalRenderer AnsiPresenter;          // DeviceAnsiStream: the presenter the frames' streams go to
    public bool DeviceAnsiDelta;                              // DeviceAnsiStream: delta streams between keyframes
    // The default is the gap with the fewest total bytes over the resting sequence of profiles/ansi_delta_rate.json (config 4, 1921 x 541,
    // frames 1..60): 3, with 1 117 018 bytes in 59 deltas; gaps 2..5 lie within 0.4 % of it, gap 0 is 2.6 % above.
    public int AnsiMergeGap = 3;
    public bool AnsiTrueColor = false;                        // DeviceAnsiStream: 24-bit colour streams
    // 0 is the exact form and stays the default until profiles/ansi_rgb_rate.json has numbers that argue otherwise (INTEGRATION.md 8.2).
    public int AnsiRgbTolerance = 0;
    public bool QuadrantGlyphs = false;                       // DeviceAnsiStream: quadrant block glyphs, 2 x 2 sub-cells a cell (superSample even, no FrameLate)
    public int QuadrantMinContrast = 0;                       // ... a cell stays one colour while its sub-cell bytes lie this close to their mean (0..255)
    public bool SixelGraphics = false;                        // DeviceAnsiStream: the frame as a sixel stream, a pixel a hi-res sample (any superSample, no FrameLate, no delta)
    public bool SixelDither = false;                          // ... with the ordered 4 x 4 dither of the quantiser
    public bool SixelDelta = false;                           // ... and as delta streams: only the bands and columns that changed are repainted
    public bool SixelAdaptivePalette = false;                 // ... under an adaptive palette of up to 256 median-cut registers in place of the cube (no dither, no delta)
    public bool SixelHoldPalette = false;                     // ... which is kept from frame to frame (hold = 1) until SixelRebuildPalette() asks for a new one
    public HipGeneratedWorld GeneratedWorld;                  // chunks that come from the generator are made on the device (ycge_scene_generate_grids)
}

/// <summary>The chunks of a voxel world that no world file holds (WorldManager.AttachChunkFromGenerator, WorldManager.cs:754-793), for a host
/// that lets the device generate them: the host keeps `Desired` at the chunk keys of its view that come from the generator (LoadChunksAround's
/// desired set less the chunks it attaches from a file or its cache as VolumeGrids) and does NOT call WorldGenerator.GenerateChunkCells for
/// them; HipRaytraceWrapper.SyncVolumeGrids generates and attaches the keys that are new, shows them as Scene.Objects' last entries and gives
/// back the slots of the keys that left.  A chunk of nothing but Air takes no slot (index -1, WorldManager.cs:759).</summary>
public sealed class HipGeneratedWorld
{
    public YWorld World;                                      // WorldConfig: ChunkSize, ChunksY, WorldSeed, WorldMin, VoxelSize
    public Func<int, int, Material> MaterialLookup;           // VolumeGrid's materialLookup: its materials must be materials of the uploaded scene
    public bool Wireframe = true;                             // VolumeGrid ctor defaults
    public float WireWidthFraction = 0.06f, WireMaxDistance = 16.0f;
    public readonly HashSet<(int cx, int cy, int cz)> Desired = new HashSet<(int cx, int cy, int cz)>();
}

/// <summary>ANSITerminalRenderer with the cell walk moved to the GPU (HipRaytraceOptions.DeviceAnsiStream): Render() writes the stream of the
/// last frame to stdout.  A frame's bytes are built by ycge_render_frame_ansi: byte for byte what ANSITerminalRenderer.Render() writes for the
/// same cells.  With HipRaytraceOptions.DeviceAnsiDelta they are built by ycge_render_frame_ansi_delta: that same stream for a keyframe (the
/// first frame, after a resize, after another geometry), otherwise only the cells that changed since the frame before, which leave the
/// terminal - cells, cursor and colours - as the full stream would.  Every frame handed over must be written, in order: Render() does.
/// With HipRaytraceOptions.AnsiTrueColor the same streams carry 24-bit colour (ycge_render_frame_ansi_rgb / _rgb_delta); the presenter writes
/// them as they are, and a wrapper of the other colour form on the same context starts with a keyframe - the library sees to that.
/// A change of console size is handled as ANSITerminalRenderer does it: onResize(width, height), and the next frame written starts with
/// ESC[2J ESC[H.  AddFrameBuffer / RemoveFrameBuffer keep the list as ANSITerminalRenderer does (:56-65); the wrapper that draws a frame hands
/// the framebuffers beside its own to the library (HipConsoleLayers), which composes them as GetChexelForPoint does.</summary>
public sealed class DeviceAnsiTerminalRenderer : ITerminalRenderer
{
    public delegate ReadOnlySpan<byte> FrameSource();
    private readonly Action<int, int> onResize;
    private readonly Stream stdout;
    public int consoleWidth { get; private set; }
    public int consoleHeight { get; private set; }
    public readonly ConsoleColor DefaultFg, DefaultBg;
    internal bool ClearPending;                 // the console changed size: the next stream starts with ESC[2J ESC[H (:100-103)
    internal FrameSource Source;                // the wrapper's last frame (HipRaytraceWrapper.LastAnsiFrame)

    public DeviceAnsiTerminalRenderer(Action<int, int> onResize)
    {
        this.onResize = onResize;
        consoleWidth = Console.WindowWidth;                                 // ANSITerminalRenderer.cs:31-37
        consoleHeight = Console.WindowHeight - 1;
        DefaultFg = Console.ForegroundColor;
        DefaultBg = Console.BackgroundColor;
        Console.CursorVisible = false;
        stdout = Console.OpenStandardOutput();
        byte[] hide = { 0x1B, (byte)'[', (byte)'?', (byte)'2', (byte)'5', (byte)'l' };      // ESC[?25l (:52-54)
        stdout.Write(hide, 0, hide.Length);
        stdout.Flush();
    }

    internal readonly List<Framebuffer> FrameBuffers = new List<Framebuffer>();      // frameBuffers (:21), bottom first

    public void AddFrameBuffer(Framebuffer fb) { FrameBuffers.Add(fb); }
    public void RemoveFrameBuffer(Framebuffer fb) { FrameBuffers.Remove(fb); }

    public void Render()
    {
        if (Console.WindowWidth != consoleWidth || Console.WindowHeight - 1 != consoleHeight)
        {
            consoleWidth = Console.WindowWidth;                             // :88-96
            consoleHeight = Console.WindowHeight - 1;
            onResize?.Invoke(consoleWidth, consoleHeight);
            ClearPending = true;                                            // (the frame in hand was built for the old size)
            return;
        }
        ReadOnlySpan<byte> s = Source != null ? Source() : ReadOnlySpan<byte>.Empty;
        if (s.IsEmpty) return;
        stdout.Write(s);
        stdout.Flush();
    }
}

public partial class RaytraceEntity
{
    /// <summary>Scene.Hit / Scene.Occluded on the GPU's copy of the active scene when the renderer is a HipRaytraceWrapper, else null
    /// (the host then keeps calling Scene.Hit).  INTEGRATION.md section 6.</summary>
    internal HipSceneQuery SceneQueries => (renderer as HipRaytraceWrapper)?.SceneQueries;

    private sealed unsafe class HipRaytraceWrapper : IConsoleRenderer, IDisposable
    {
        private IntPtr ctx;
        private readonly Scene scene;
        private int fbW, fbH, ss;
        private float fov;
        private Vec3 pos; private float yaw, pitch;
        private float* sdr;                         // fbW * fbH * {top rgb, bottom rgb}: page-locked memory of the library (ycge_alloc_host_buffer)
        private float* sdrLate;                     // FrameLate: the second array - the frame in flight fills one while the host blits the other
        private readonly bool frameLate;
        private readonly bool deviceColors;         // DeviceChexelColors: color16 / color16Late hold {color_16 of top | of bottom << 4} per chexel
        private byte* color16, color16Late;         // (page-locked memory of the library, one per SDR array)
        private readonly DeviceAnsiTerminalRenderer ansi;       // DeviceAnsiStream: the presenter of the streams
        private byte* ansiBuf;                      // the last frame's stream (page-locked memory of the library, ansiCap bytes)
        private ulong ansiCap, ansiLen;
        private byte* ansiBufLate;                  // FrameLate: the second stream buffer - the frame in flight fills one while the presenter writes the other
        private ulong ansiCapLate;
        private YAnsiAsyncResult* ansiRec, ansiRecLate;   // FrameLate: the records of the two (page-locked memory of the library)
        private readonly bool ansiDelta;            // DeviceAnsiDelta: delta streams between keyframes
        private readonly int ansiMergeGap;
        private bool ansiRgb;                       // AnsiTrueColor: the 24-bit colour forms of the two calls
        private readonly int ansiTolerance;
        private readonly bool ansiQuad;             // QuadrantGlyphs: the quadrant-glyph forms of the two calls
        private readonly int ansiMinContrast;
        private readonly bool sixel, sixelDither;   // SixelGraphics: ycge_render_frame_sixel in place of every stream form
        private readonly bool sixelDelta;           // ... SixelDelta: ycge_render_frame_sixel_delta
        private readonly bool sixelPalette, sixelHold;   // ... SixelAdaptivePalette / SixelHoldPalette: ycge_render_frame_sixel_palette
        private bool sixelRebuild;                  // ... the next frame builds its palette whatever sixelHold says
        private bool sixelBufOwned;                 // ... ansiBuf is pageable memory of this wrapper (Marshal), not the library's page-locked memory
        private bool inFlight;                      // FrameLate: a frame queued by the last TryFlipAndBlit has not been waited for yet
        private FlatScene uploaded;                 // what the device holds (records only; its pins are released after the upload)
        private ulong objectsSignature;
        private bool forceUpload;
        private readonly HipGeneratedWorld generated;                   // HipRaytraceOptions.GeneratedWorld (null: every chunk is a VolumeGrid of the host)
        private readonly Dictionary<(int, int, int), int> generatedIndex = new Dictionary<(int, int, int), int>();   // key -> device grid index, -1: all Air
        private YLight[] lightsSent = Array.Empty<YLight>();
        private YVec3 ambientSent, topSent, bottomSent; private float ambientIntensitySent;

        public HipRaytraceWrapper(Framebuffer fb, Scene scene, float fovDeg, int superSample, HipRaytraceOptions options = null)
        {
            this.scene = scene ?? throw new ArgumentNullException(nameof(scene));
            var cfg = new YConfig();
            Ycge.Check(IntPtr.Zero, Ycge.ycge_config_default(ref cfg));
            cfg.FbWidth = fbW = fb.Width; cfg.FbHeight = fbH = fb.Height; cfg.SuperSample = ss = Math.Max(1, superSample); cfg.FovDeg = fov = fovDeg;
            if (options?.Devices != null && options.Devices.Length > 0)
            {
                if (options.Devices.Length > 8) throw new ArgumentException("at most 8 devices (YCGE_MAX_DEVICES)");
                cfg.NDevices = options.Devices.Length;
                for (int i = 0; i < options.Devices.Length; i++) cfg.Devices[i] = options.Devices[i];
                cfg.MultiDeviceExchange = (int)options.Exchange;
            }
            ansi = options != null && options.DeviceAnsiStream ? options.AnsiPresenter ?? throw new ArgumentException("DeviceAnsiStream needs an AnsiPresenter") : null;
            ansiDelta = ansi != null && options.DeviceAnsiDelta; ansiMergeGap = options != null ? options.AnsiMergeGap : 3;
            ansiRgb = ansi != null && options.AnsiTrueColor; ansiTolerance = options != null ? options.AnsiRgbTolerance : 0;
            ansiQuad = ansi != null && options.QuadrantGlyphs; ansiMinContrast = options != null ? options.QuadrantMinContrast : 0;
            if (ansiQuad && (ss & 1) != 0) throw new ArgumentException("QuadrantGlyphs needs an even superSample");
            if (ansiQuad && options.FrameLate) throw new ArgumentException("QuadrantGlyphs has no FrameLate form");
            ansiRgb |= ansiQuad;                    // (the quadrant streams are 24-bit ones: their bound is the 24-bit bound)
            sixel = ansi != null && options.SixelGraphics; sixelDither = sixel && options.SixelDither; sixelDelta = sixel && options.SixelDelta;
            if (sixel && (options.FrameLate || options.DeviceAnsiDelta || options.QuadrantGlyphs)) throw new ArgumentException("SixelGraphics has no FrameLate, delta or quadrant form");
            sixelPalette = sixel && options.SixelAdaptivePalette; sixelHold = sixelPalette && options.SixelHoldPalette;
            if (sixelPalette && (sixelDither || sixelDelta)) throw new ArgumentException("SixelAdaptivePalette has no dither and no delta form");
            frameLate = options != null && options.FrameLate && cfg.NDevices <= 1;      // (frames in flight are the single-device form)
            deviceColors = options != null && options.DeviceChexelColors;
            generated = options?.GeneratedWorld;
            Ycge.Check(IntPtr.Zero, Ycge.ycge_create(ref cfg, out ctx));
            AllocSdr();
            Upload();                               // the reference ctor ends with scene.RebuildBVH() (RaytraceRenderer.cs:107)
            if (ansi != null) ansi.Source = () => LastAnsiFrame;
        }

        /// <summary>DeviceAnsiStream: the bytes of the last frame, as ANSITerminalRenderer.Render() writes them (valid until the next frame).</summary>
        public ReadOnlySpan<byte> LastAnsiFrame => ansiBuf == null ? ReadOnlySpan<byte>.Empty : new ReadOnlySpan<byte>(ansiBuf, checked((int)ansiLen));

        // FrameLate: the stream queued by the last call is finished first and becomes LastAnsiFrame; the other buffer and record are free again
        private void FinishAnsiInFlight()
        {
            if (!inFlight) return;
            Ycge.Check(ctx, Ycge.ycge_wait(ctx)); inFlight = false;
            byte* b = ansiBuf; ansiBuf = ansiBufLate; ansiBufLate = b;
            ulong cap = ansiCap; ansiCap = ansiCapLate; ansiCapLate = cap;
            YAnsiAsyncResult* r = ansiRec; ansiRec = ansiRecLate; ansiRecLate = r;
            if (ansiRec->Status != 0) throw new InvalidOperationException("the device ANSI stream exceeded its buffer; nothing was copied");
            ansiLen = ansiRec->Length;
        }

        // FrameLate: this call's frame queued into the second buffer (grown to the stream's bound: nothing is in flight), one frame late
        private void QueueAnsi(Framebuffer fb, int cw, int ch, UIntPtr bound)
        {
            if ((ulong)bound > ansiCapLate)
            {
                if (ansiBufLate != null) { Ycge.ycge_free_host_buffer((IntPtr)ansiBufLate); ansiBufLate = null; ansiCapLate = 0; }
                Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(bound, out IntPtr p));
                ansiBufLate = (byte*)p; ansiCapLate = (ulong)bound;
            }
            if (ansiRec == null)
            {
                Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer((UIntPtr)sizeof(YAnsiAsyncResult), out IntPtr r0)); ansiRec = (YAnsiAsyncResult*)r0;
                Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer((UIntPtr)sizeof(YAnsiAsyncResult), out IntPtr r1)); ansiRecLate = (YAnsiAsyncResult*)r1;
            }
            if (ansi.ClearPending) ansiLen = 0;                                 // (the frame in hand was built for the old console; a keyframe follows)
            var req = new YAnsiAsync { ConsoleW = cw, ConsoleH = ch, ViewportX = fb.ViewportX, ViewportY = fb.ViewportY, DefaultFg16 = (int)ansi.DefaultFg,
                                       DefaultBg16 = (int)ansi.DefaultBg, ClearScreen = ansi.ClearPending ? 1 : 0, Rgb = ansiRgb ? 1 : 0, Delta = ansiDelta ? 1 : 0,
                                       MergeGap = ansiDelta ? ansiMergeGap : 0, Tolerance = ansiDelta && ansiRgb ? ansiTolerance : 0, Keyframe = 0 };
            Ycge.Check(ctx, Ycge.ycge_render_frame_async_ansi(ctx, &req, ansiBufLate, (UIntPtr)ansiCapLate, ansiRecLate, null));
            inFlight = true;
            ansi.ClearPending = false;
        }

        // one frame into the stream of the presenter's console (the framebuffer at its viewport), the buffer grown to the stream's bound
        private void RenderAnsi(Framebuffer fb)
        {
            int cw = ansi.consoleWidth, ch = ansi.consoleHeight;
            UIntPtr bound;
            if (sixel) { RenderSixel(fb); return; }
            if (ansiRgb) Ycge.Check(ctx, Ycge.ycge_ansi_rgb_stream_bound(cw, ch, out bound));
            else Ycge.Check(ctx, Ycge.ycge_ansi_stream_bound(cw, ch, out bound));
            if (frameLate)
            {
                HipConsoleLayers.Set(ctx, ansi.FrameBuffers, fb);               // (joins: TryFlipAndBlit has waited for the frame in flight already)
                QueueAnsi(fb, cw, ch, bound);
                return;
            }
            if ((ulong)bound > ansiCap)
            {
                FreeAnsiBuf();
                Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(bound, out IntPtr p));
                ansiBuf = (byte*)p; ansiCap = (ulong)bound;
            }
            HipConsoleLayers.Set(ctx, ansi.FrameBuffers, fb);                   // (the other framebuffers as they stand now; fb is this wrapper's own)
            UIntPtr len;
            if (ansiQuad && ansiDelta)
                Ycge.Check(ctx, Ycge.ycge_render_frame_ansi_quad_delta(ctx, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg, ansi.ClearPending ? 1 : 0,
                                                                       ansiMergeGap, ansiTolerance, 0, ansiMinContrast, ansiBuf, (UIntPtr)ansiCap, &len, null, null, null));
            else if (ansiQuad)
                Ycge.Check(ctx, Ycge.ycge_render_frame_ansi_quad(ctx, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg, ansi.ClearPending ? 1 : 0,
                                                                 ansiMinContrast, ansiBuf, (UIntPtr)ansiCap, &len, null, null));
            else if (ansiRgb && ansiDelta)
                Ycge.Check(ctx, Ycge.ycge_render_frame_ansi_rgb_delta(ctx, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg, ansi.ClearPending ? 1 : 0,
                                                                      ansiMergeGap, ansiTolerance, 0, ansiBuf, (UIntPtr)ansiCap, &len, null, null, null));
            else if (ansiRgb)
                Ycge.Check(ctx, Ycge.ycge_render_frame_ansi_rgb(ctx, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg, ansi.ClearPending ? 1 : 0,
                                                                ansiBuf, (UIntPtr)ansiCap, &len, null, null));
            else if (ansiDelta)
                Ycge.Check(ctx, Ycge.ycge_render_frame_ansi_delta(ctx, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg, ansi.ClearPending ? 1 : 0,
                                                                  ansiMergeGap, 0, ansiBuf, (UIntPtr)ansiCap, &len, null, null, null));
            else
                Ycge.Check(ctx, Ycge.ycge_render_frame_ansi(ctx, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg, ansi.ClearPending ? 1 : 0,
                                                            ansiBuf, (UIntPtr)ansiCap, &len, null, null));
            ansiLen = (ulong)len;
            ansi.ClearPending = false;
        }

        /// <summary>SixelHoldPalette: the next frame builds a new palette from its picture (a cut, a new scene, every N frames)</summary>
        public void SixelRebuildPalette() { sixelRebuild = true; }

        // SixelGraphics: one frame as the sixel stream of its hi-res samples at the framebuffer's viewport.  The bound is large against the streams
        // (74 MB for 1920 x 1072 pixels, streams of a few hundred KB): the buffer is pageable, so only the pages a stream reaches are ever backed
        private void RenderSixel(Framebuffer fb)
        {
            UIntPtr bound;
            if (sixelPalette) Ycge.Check(ctx, Ycge.ycge_sixel_palette_stream_bound(fbW * ss, 2 * fbH * ss, out bound));
            else Ycge.Check(ctx, Ycge.ycge_sixel_stream_bound(fbW * ss, 2 * fbH * ss, out bound));
            if ((ulong)bound > ansiCap)
            {
                FreeAnsiBuf();
                ansiBuf = (byte*)System.Runtime.InteropServices.Marshal.AllocHGlobal(checked((IntPtr)(long)(ulong)bound)); sixelBufOwned = true; ansiCap = (ulong)bound;
            }
            UIntPtr len;
            if (sixelPalette)
            {
                Ycge.Check(ctx, Ycge.ycge_render_frame_sixel_palette(ctx, fb.ViewportX, fb.ViewportY, ansi.ClearPending ? 1 : 0, sixelHold && !sixelRebuild ? 1 : 0, ansiBuf,
                                                                     (UIntPtr)ansiCap, &len, null, null, null, null));
                sixelRebuild = false;
            }
            else if (sixelDelta)
                Ycge.Check(ctx, Ycge.ycge_render_frame_sixel_delta(ctx, fb.ViewportX, fb.ViewportY, ansi.ClearPending ? 1 : 0, 0, sixelDither ? 1 : 0, ansiBuf, (UIntPtr)ansiCap, &len,
                                                                   null, null, null));
            else
                Ycge.Check(ctx, Ycge.ycge_render_frame_sixel(ctx, fb.ViewportX, fb.ViewportY, ansi.ClearPending ? 1 : 0, sixelDither ? 1 : 0, ansiBuf, (UIntPtr)ansiCap, &len, null, null));
            ansiLen = (ulong)len;
            ansi.ClearPending = false;
        }

        private void FreeAnsiBuf()
        {
            if (ansiBuf == null) return;
            if (sixelBufOwned) System.Runtime.InteropServices.Marshal.FreeHGlobal((IntPtr)ansiBuf); else Ycge.ycge_free_host_buffer((IntPtr)ansiBuf);
            ansiBuf = null; sixelBufOwned = false; ansiCap = ansiLen = 0;
        }

        /// <summary>What the devices' tiles really travel by (the library falls back to the peer push where librccl.so is missing).</summary>
        public YExchange ExchangeInUse { get { Ycge.Check(ctx, Ycge.ycge_exchange_query(ctx, out int mode, out _)); return (YExchange)mode; } }

        private void AllocSdr()
        {
            if (sdr != null || sdrLate != null) { Ycge.ycge_wait(ctx); if (inFlight && ansi != null) ansiLen = 0; inFlight = false; }      // (a queued stream nobody wrote: the next one is a keyframe, ycge_resize sees to that)
            if (sdr != null) { Ycge.ycge_free_host_buffer((IntPtr)sdr); sdr = null; }
            if (sdrLate != null) { Ycge.ycge_free_host_buffer((IntPtr)sdrLate); sdrLate = null; }
            FreeColor16();
            UIntPtr bytes = (UIntPtr)((ulong)fbW * (ulong)fbH * 6 * sizeof(float));
            Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(bytes, out IntPtr p));
            sdr = (float*)p;
            if (frameLate) { Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(bytes, out IntPtr q)); sdrLate = (float*)q; }
            if (deviceColors)
            {
                UIntPtr cbytes = (UIntPtr)((ulong)fbW * (ulong)fbH);
                Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(cbytes, out IntPtr c)); color16 = (byte*)c;
                if (frameLate) { Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(cbytes, out IntPtr d)); color16Late = (byte*)d; }
            }
        }

        private void FreeColor16()
        {
            if (color16 != null) { Ycge.ycge_free_host_buffer((IntPtr)color16); color16 = null; }
            if (color16Late != null) { Ycge.ycge_free_host_buffer((IntPtr)color16Late); color16Late = null; }
        }

        // ---- scene: full upload, and what changes between frames (Scene.Update: entities move objects, DayNightCycle.cs:80-89 moves lights and sky)
        private void Upload()
        {
            uploaded?.Dispose();
            uploaded = SceneFlattener.Flatten(scene);
            YScene s = uploaded.Scene;
            Ycge.Check(ctx, Ycge.ycge_scene_upload(ctx, ref s));
            uploaded.Dispose();                     // (frees pins and unmanaged copies; the record arrays and owner lists stay readable)
            objectsSignature = ObjectsSignature();
            RememberLights(uploaded.Lights);
        }

        private ulong ObjectsSignature()
        {
            // identity and bounds of every object, in order: an entity that moves, adds or removes geometry changes it (Scene.cs:122-127)
            ulong h = 1469598103934665603UL;
            void Mix(uint v) { h = (h ^ v) * 1099511628211UL; }
            foreach (Hittable o in scene.Objects)
            {
                Mix((uint)RuntimeHelpers.GetHashCode(o));
                if (o.TryGetBounds(out float a, out float b, out float c, out float d, out float e, out float f, out _, out _, out _))
                { Mix(BitConverter.SingleToUInt32Bits(a)); Mix(BitConverter.SingleToUInt32Bits(b)); Mix(BitConverter.SingleToUInt32Bits(c)); Mix(BitConverter.SingleToUInt32Bits(d)); Mix(BitConverter.SingleToUInt32Bits(e)); Mix(BitConverter.SingleToUInt32Bits(f)); }
            }
            return h;
        }

        private void RememberLights(YLight[] l)
        {
            lightsSent = l; ambientSent = new YVec3(scene.Ambient.Color); ambientIntensitySent = scene.Ambient.Intensity;
            topSent = new YVec3(scene.BackgroundTop); bottomSent = new YVec3(scene.BackgroundBottom);
        }
        private static bool Same(YVec3 a, YVec3 b) => a.X.Equals(b.X) && a.Y.Equals(b.Y) && a.Z.Equals(b.Z);
        private static bool Same(YLight[] a, YLight[] b)
        {
            if (a.Length != b.Length) return false;
            for (int i = 0; i < a.Length; i++) if (!Same(a[i].Position, b[i].Position) || !Same(a[i].Color, b[i].Color) || !a[i].Intensity.Equals(b[i].Intensity)) return false;
            return true;
        }

        /// <summary>Chunk streaming (WorldManager.LoadChunksAround, WorldManager.cs:289-370): the scene's VolumeGrids that the device does not
        /// hold yet are attached (ycge_scene_attach_grids: their cells go up once and are encoded on the device).  False when one of them
        /// needs a material the last upload did not hold.</summary>
        internal bool SyncVolumeGrids(Scene scene)
        {
            var fresh = new List<VolumeGrid>();
            foreach (Hittable o in scene.Objects) if (o is VolumeGrid g && !uploaded.GridOwners.Contains(g)) fresh.Add(g);
            if (fresh.Count == 0) return true;
            using (var scratch = new FlatScene())
            {
                var records = new YGrid[fresh.Count];
                for (int i = 0; i < records.Length; i++) if (!SceneFlattener.FlattenGrid(fresh[i], uploaded, scratch, out records[i])) return false;
                var index = new int[records.Length];
                fixed (YGrid* r = records) fixed (int* ix = index) Ycge.Check(ctx, Ycge.ycge_scene_attach_grids(ctx, r, records.Length, ix));
                for (int i = 0; i < index.Length; i++)
                {
                    while (uploaded.GridOwners.Count <= index[i]) uploaded.GridOwners.Add(null);
                    uploaded.GridOwners[index[i]] = fresh[i];
                }
            }
            return true;
        }

        /// <summary>Meshes of a running scene (an entity whose GetHittables() yields a Mesh, Scene.cs:519-535): the scene's Meshes that the
        /// device does not hold yet are attached (ycge_scene_attach_meshes: only their own trees are built and their records written), the
        /// materials they bring appended first (ycge_scene_append_materials).  False when one of them needs a texture the last upload did not hold.</summary>
        internal bool SyncMeshes(Scene scene)
        {
            var fresh = new List<Mesh>();
            foreach (Hittable o in scene.Objects) if (o is Mesh m && !uploaded.MeshOwners.Contains(m) && !fresh.Contains(m)) fresh.Add(m);
            if (fresh.Count == 0) return true;
            using (var scratch = new FlatScene())
            {
                var records = new YMesh[fresh.Count];
                for (int i = 0; i < records.Length; i++)
                {
                    if (!SceneFlattener.FlattenMesh(fresh[i], uploaded, scratch, out records[i], out YMaterial[] added)) return false;
                    if (added.Length == 0) continue;
                    int first;
                    fixed (YMaterial* a = added) Ycge.Check(ctx, Ycge.ycge_scene_append_materials(ctx, a, added.Length, &first));
                    if (first != uploaded.Materials.Length) throw new InvalidOperationException("ycge_scene_append_materials numbered the materials differently");
                    var longer = new YMaterial[uploaded.Materials.Length + added.Length];
                    uploaded.Materials.CopyTo(longer, 0); added.CopyTo(longer, uploaded.Materials.Length);
                    uploaded.Materials = longer;
                }
                var index = new int[records.Length];
                fixed (YMesh* r = records) fixed (int* ix = index) Ycge.Check(ctx, Ycge.ycge_scene_attach_meshes(ctx, r, records.Length, ix));
                for (int i = 0; i < index.Length; i++)
                {
                    while (uploaded.MeshOwners.Count <= index[i]) uploaded.MeshOwners.Add(null);
                    uploaded.MeshOwners[index[i]] = fresh[i];
                }
            }
            return true;
        }

        /// <summary>... and the meshes that left Scene.Objects give their indices back (after ycge_scene_update_objects: nothing refers to them).</summary>
        private void DetachMeshes()
        {
            var live = new HashSet<Mesh>();
            foreach (Hittable o in scene.Objects) if (o is Mesh m) live.Add(m);
            var gone = new List<int>();
            for (int i = 0; i < uploaded.MeshOwners.Count; i++) if (uploaded.MeshOwners[i] != null && !live.Contains(uploaded.MeshOwners[i])) gone.Add(i);
            if (gone.Count == 0) return;
            int[] ix = gone.ToArray();
            fixed (int* p = ix) Ycge.Check(ctx, Ycge.ycge_scene_detach_meshes(ctx, p, ix.Length));
            foreach (int i in gone) uploaded.MeshOwners[i] = null;
        }

        /// <summary>Chunks that came from the generator (HipGeneratedWorld): the desired keys the device does not hold yet are generated ON
        /// THE DEVICE and attached in one call (ycge_scene_generate_grids: keys in, device indices back, -1 for a chunk of nothing but Air,
        /// which gets no object); no cells are made or sent by the host.  False when the lookup needs a material the last upload did not hold.</summary>
        private bool SyncGeneratedChunks()
        {
            if (generated == null) return true;
            var fresh = new List<(int, int, int)>();
            foreach (var key in generated.Desired) if (!generatedIndex.ContainsKey(key)) fresh.Add(key);
            if (fresh.Count == 0) return true;
            using (var scratch = new FlatScene())
            {
                if (!SceneFlattener.GeneratorProto(generated, uploaded, scratch, out YGrid proto)) return false;
                var keys = new int[3 * fresh.Count];
                for (int i = 0; i < fresh.Count; i++) { keys[3 * i] = fresh[i].Item1; keys[3 * i + 1] = fresh[i].Item2; keys[3 * i + 2] = fresh[i].Item3; }
                var index = new int[fresh.Count];
                YWorld world = generated.World;
                fixed (int* k = keys) fixed (int* ix = index) Ycge.Check(ctx, Ycge.ycge_scene_generate_grids(ctx, ref world, k, fresh.Count, &proto, ix, null));
                for (int i = 0; i < index.Length; i++) generatedIndex[fresh[i]] = index[i];
            }
            return true;
        }
        private bool GeneratedChanged()
        {
            if (generated == null) return false;
            if (generated.Desired.Count != generatedIndex.Count) return true;
            foreach (var key in generated.Desired) if (!generatedIndex.ContainsKey(key)) return true;
            return false;
        }
        /// <summary>Scene.Objects' records followed by one VolumeGrid record per resident generated chunk that is still desired (they have no
        /// host object: the reference would have scene.Add'ed their VolumeGrids last, WorldManager.cs:775).</summary>
        private YPrim[] WithGenerated(YPrim[] prims)
        {
            if (generated == null || prims == null) return prims;
            var all = new List<YPrim>(prims);
            foreach (var kv in generatedIndex)
                if (kv.Value >= 0 && generated.Desired.Contains(kv.Key)) all.Add(new YPrim { Type = (int)YPrimType.VolumeGrid, Ref = kv.Value });
            return all.ToArray();
        }

        /// <summary>... and the grids that left Scene.Objects give their slots back (after ycge_scene_update_objects: nothing refers to them).</summary>
        private void DetachVolumeGrids()
        {
            var live = new HashSet<VolumeGrid>();
            foreach (Hittable o in scene.Objects) if (o is VolumeGrid g) live.Add(g);
            var gone = new List<int>();
            for (int i = 0; i < uploaded.GridOwners.Count; i++) if (uploaded.GridOwners[i] != null && !live.Contains(uploaded.GridOwners[i])) gone.Add(i);
            if (generated != null)          // generated chunks that left the view: their slots go back too (a -1 held none)
            {
                var left = new List<(int, int, int)>();
                foreach (var kv in generatedIndex) if (!generated.Desired.Contains(kv.Key)) { left.Add(kv.Key); if (kv.Value >= 0) gone.Add(kv.Value); }
                foreach (var key in left) generatedIndex.Remove(key);
            }
            if (gone.Count == 0) return;
            int[] ix = gone.ToArray();
            fixed (int* p = ix) Ycge.Check(ctx, Ycge.ycge_scene_detach_grids(ctx, p, ix.Length));
            foreach (int i in gone) if (i < uploaded.GridOwners.Count) uploaded.GridOwners[i] = null;
        }

        private void SyncScene()
        {
            if (forceUpload || ObjectsSignature() != objectsSignature || GeneratedChanged())
            {
                YPrim[] prims = forceUpload || !SyncVolumeGrids(scene) || !SyncMeshes(scene) || !SyncGeneratedChunks() ? null : WithGenerated(SceneFlattener.ObjectsAgainst(scene, uploaded));
                forceUpload = false;
                if (prims == null)
                {
                    Upload();                       // a new texture, or a new material on an object that is no mesh: the whole scene again
                    generatedIndex.Clear();         // (an upload forgets every attached grid; the generated chunks are made again)
                    if (generated != null && generated.Desired.Count > 0)
                    {
                        if (!SyncGeneratedChunks()) throw new InvalidOperationException("HipGeneratedWorld.MaterialLookup returns a material the scene does not hold");
                        prims = WithGenerated(uploaded.Prims);
                        fixed (YPrim* p = prims) Ycge.Check(ctx, Ycge.ycge_scene_update_objects(ctx, p, prims.Length));
                        uploaded.Prims = prims;
                    }
                }
                else
                {
                    fixed (YPrim* p = prims) Ycge.Check(ctx, Ycge.ycge_scene_update_objects(ctx, p, prims.Length));     // only the scene-level BVH is rebuilt, as in the reference
                    uploaded.Prims = prims;
                    DetachVolumeGrids();
                    DetachMeshes();
                    objectsSignature = ObjectsSignature();
                }
            }
            YLight[] lights = SceneFlattener.LightRecords(scene);
            YVec3 amb = new YVec3(scene.Ambient.Color), top = new YVec3(scene.BackgroundTop), bot = new YVec3(scene.BackgroundBottom);
            if (!Same(lights, lightsSent) || !Same(amb, ambientSent) || !Same(top, topSent) || !Same(bot, bottomSent) || !scene.Ambient.Intensity.Equals(ambientIntensitySent))
            {
                fixed (YLight* l = lights) Ycge.Check(ctx, Ycge.ycge_scene_update_lights(ctx, l, lights.Length, &amb, scene.Ambient.Intensity, &top, &bot));
                RememberLights(lights);
            }
            // live textures: the frame the reader shows NOW is the frame this TryFlipAndBlit samples (Renderer/Texture.cs:113-116)
            for (int i = 0; i < uploaded.Textures.Count; i++)
            {
                Texture t = uploaded.Textures[i];
                if (!SceneFlattenerAccess.IsDynamic(t)) continue;
                IntPtr frame = SceneFlattenerAccess.CurrentFrame(t, out int bpp);
                if (frame != IntPtr.Zero) Ycge.Check(ctx, Ycge.ycge_scene_update_texture(ctx, i, frame, (UIntPtr)((ulong)t.width * (ulong)t.height * (ulong)bpp)));
            }
        }

        /// <summary>The native context, for the scene queries (HipSceneQuery): they answer against the scene as the last SyncScene left it.</summary>
        internal IntPtr NativeContext => ctx;
        private HipSceneQuery queries;
        /// <summary>Scene.Hit / Scene.Occluded on the device scene of this wrapper (VolumeScene's camera physics; INTEGRATION.md section 6).</summary>
        internal HipSceneQuery SceneQueries => queries ??= new HipSceneQuery(() => ctx);
        /// <summary>VolumeScene's camera physics on the device scene (HipVolumeCamera): one ycge_volume_camera_tick a tick instead of a query a ray.</summary>
        internal HipVolumeCamera NewVolumeCamera(Vec3 cameraPos, float worldHeight, float waterLevel, float voxelSizeY, bool autoPlaced)
            => new HipVolumeCamera(() => ctx, cameraPos, worldHeight, waterLevel, voxelSizeY, autoPlaced);
        /// <summary>The other bodies of a voxel world - mobs, items, projectiles, replicated players - on the device scene (HipVolumeBodies): one ycge_volume_bodies_tick a tick for all of them.</summary>
        internal HipVolumeBodies NewVolumeBodies(float worldHeight, float waterLevel, float voxelSizeY)
            => new HipVolumeBodies(() => ctx, worldHeight, waterLevel, voxelSizeY);

        /// <summary>Forces the next frame to upload the scene again (for a host that edits a scene in ways the signature cannot see).</summary>
        public void Invalidate() { forceUpload = true; }

        // ---- IConsoleRenderer
        public void SetCamera(Vec3 p, float y, float pt) { pos = p; yaw = y; pitch = pt; Push(); }
        public void SetFov(float f) { fov = f; Push(); }
        private void Push()
        {
            float* p = stackalloc float[3] { pos.X, pos.Y, pos.Z };
            Ycge.Check(ctx, Ycge.ycge_set_camera(ctx, p, yaw, pitch, fov));
        }

        public void Resize(Framebuffer fb, int superSample)
        {
            fbW = fb.Width; fbH = fb.Height; ss = Math.Max(1, superSample);
            Ycge.Check(ctx, Ycge.ycge_resize(ctx, fbW, fbH, ss));          // drops the TAA history (RaytraceRenderer.cs:137)
            AllocSdr();
        }

        public void TryFlipAndBlit(Framebuffer fb)
        {
            if (fb.Width != fbW || fb.Height != fbH) Resize(fb, ss);       // RaytraceRenderer.cs:119-120 does the same check
            if (ansi != null)
            {
                if (frameLate) FinishAnsiInFlight();                           // (it ran beside the host's Update and the presenter's write in between)
                SyncScene();
                RenderAnsi(fb);                                                // (the presenter writes the stream: no chexel reaches the framebuffer)
                return;
            }
            if (frameLate)
            {
                // the frame queued by the LAST call is finished first (it ran beside the host's Update in between), then this call's frame is queued
                // into the other array and the finished one is blitted: one frame late, never torn (the device writes `sdrLate`, the host reads `sdr`)
                bool have = inFlight;
                if (inFlight)
                {
                    Ycge.Check(ctx, Ycge.ycge_wait(ctx)); inFlight = false;
                    float* t = sdr; sdr = sdrLate; sdrLate = t;
                    byte* u = color16; color16 = color16Late; color16Late = u;
                }
                SyncScene();
                if (deviceColors) Ycge.Check(ctx, Ycge.ycge_render_frame_async_chexels(ctx, sdrLate, color16Late, null, null));
                else Ycge.Check(ctx, Ycge.ycge_render_frame_async_sdr(ctx, sdrLate));
                inFlight = true;
                if (!have) return;                                             // (the very first call has nothing to show yet: the framebuffer keeps what it had)
            }
            else
            {
                SyncScene();
                if (deviceColors) Ycge.Check(ctx, Ycge.ycge_render_frame_chexels(ctx, sdr, color16, null, null, null));
                else Ycge.Check(ctx, Ycge.ycge_render_frame(ctx, sdr, null));
            }
            if (deviceColors)
            {
                // the 3-argument ChexelColor applies the same Clamp01 (Chexel.cs:49-53): only the palette search has left the host
                for (int cy = 0; cy < fbH; cy++)
                    for (int cx = 0; cx < fbW; cx++)
                    {
                        float* c = sdr + ((long)cx + (long)cy * fbW) * 6;
                        byte b = color16[(long)cx + (long)cy * fbW];
                        fb.SetChexel(cx, cy, new Chexel('▀', new ChexelColor((ConsoleColor)(b & 15), new Vec3(c[0], c[1], c[2])),
                                                             new ChexelColor((ConsoleColor)(b >> 4), new Vec3(c[3], c[4], c[5]))));
                    }
                return;
            }
            for (int cy = 0; cy < fbH; cy++)
                for (int cx = 0; cx < fbW; cx++)
                {
                    float* c = sdr + ((long)cx + (long)cy * fbW) * 6;      // {top rgb, bottom rgb}
                    fb.SetChexel(cx, cy, new Chexel('▀', new Vec3(c[0], c[1], c[2]), new Vec3(c[3], c[4], c[5])));      // RaytraceRenderer.cs:260-261
                }
        }

        public void Dispose()
        {
            if (ctx != IntPtr.Zero) { Ycge.ycge_destroy(ctx); ctx = IntPtr.Zero; }      // (waits for everything in flight)
            if (sdr != null) { Ycge.ycge_free_host_buffer((IntPtr)sdr); sdr = null; }
            if (sdrLate != null) { Ycge.ycge_free_host_buffer((IntPtr)sdrLate); sdrLate = null; }
            FreeColor16();
            FreeAnsiBuf();
            if (ansiBufLate != null) { Ycge.ycge_free_host_buffer((IntPtr)ansiBufLate); ansiBufLate = null; }
            if (ansiRec != null) { Ycge.ycge_free_host_buffer((IntPtr)ansiRec); ansiRec = null; }
            if (ansiRecLate != null) { Ycge.ycge_free_host_buffer((IntPtr)ansiRecLate); ansiRecLate = null; }
            uploaded?.Dispose();
        }
    }
}

namespace ConsoleGame.RayTracing.Native
{
    /// <summary>The two questions the wrapper asks a Texture per frame (accessor first, private field of the unmodified reference otherwise).</summary>
    internal static class SceneFlattenerAccess
    {
        private const System.Reflection.BindingFlags Any = System.Reflection.BindingFlags.Instance | System.Reflection.BindingFlags.Public | System.Reflection.BindingFlags.NonPublic;
        private static object Get(object o, params string[] names)
        {
            foreach (string n in names)
            {
                var p = o.GetType().GetProperty(n, Any); if (p != null) return p.GetValue(o);
                var f = o.GetType().GetField(n, Any); if (f != null) return f.GetValue(o);
            }
            return null;
        }
        public static bool IsDynamic(ConsoleGame.Renderer.Texture t) => Get(t, "IsDynamic", "isDynamic") is bool b && b;
        public static IntPtr CurrentFrame(ConsoleGame.Renderer.Texture t, out int bytesPerPixel)
        {
            bytesPerPixel = Get(t, "DynamicBytesPerPixel", "dynamicBytesPerPixel") is int n ? n : 0;
            return Get(t, "DynamicReader", "dynamicReader") is NullEngine.Video.IFrameReader r ? r.GetCurrentFramePtr() : IntPtr.Zero;
        }
    }
}
