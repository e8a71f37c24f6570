// HipVideoWrapper.cs - the fourth IConsoleRenderer of RaytraceEntity (RaytraceEntity.cs:12-50): VideoWrapper -> VideoRenderer with the
// Lanczos blit on the GPU.
//
// The reference's VideoRenderer owns two things: an IFrameReader (AsyncFfmpegVideoReader / AsyncCameraReader: decoding, the camera, audio)
// and TryFlipAndBlit, which resamples the reader's current frame to chexels on a pool of CPU threads (Renderer/VideoRenderer.cs:68-148).
// This wrapper keeps the reader in C# unchanged and passes its frame pointer to ycge_video_blit: the SDR values that reach
// fb.SetChexel are the reference's bit for bit.  SetCamera and SetFov are no-ops, as VideoWrapper's; Resize is ycge_resize, since
// VideoWrapper.Resize makes a new VideoRenderer for the new framebuffer (the reader is kept: no re-open).
//
// It blits through a context of its own (no scene is ever uploaded) or through the context of the HipRaytraceWrapper it replaces while
// the user is in Video mode - a blit changes nothing a ray-traced frame reads, so I / U switch back to the frame sequence as it was.
// The presenter options are HipRaytraceOptions' (HipRaytraceWrapper.cs): DeviceChexelColors reads back one byte a chexel beside the SDR and
// the host no longer searches the palette; DeviceAnsiStream hands the presenter the bytes ANSITerminalRenderer.Render() would write.
// QuadrantGlyphs + QuadrantMinContrast: the quadrant-glyph forms (ycge_video_blit_ansi_quad / _quad_delta), so that the mode switch keeps the
// glyph family and, with DeviceAnsiDelta, the quadrant family's delta state: the first video frame behind a traced one is a delta, not a keyframe.
// SixelGraphics / SixelDither / SixelDelta: the film per pixel (ycge_video_blit_sixel / _sixel_delta), so that a host with SixelGraphics on keeps
// its presenter through the mode switch; with SixelDelta a paused film costs the header and the trailer, and the first video frame behind a
// traced one is a delta.  SixelAdaptivePalette / SixelHoldPalette: the adaptive palette's form (ycge_video_blit_sixel_palette) on the palette the
// context's frames share - no dither, no delta.  INTEGRATION.md sections 8.6 and 9.
using System;
using ConsoleGame.RayTracing;
using ConsoleGame.RayTracing.Native;
using ConsoleGame.Renderer;
using NullEngine.Video;

public partial class RaytraceEntity
{
    private sealed unsafe class HipVideoWrapper : IConsoleRenderer, IDisposable
    {
        private IntPtr ctx;
        private readonly bool ownsContext;
        private readonly IFrameReader reader;
        private readonly bool useRGBA;
        private int fbW, fbH, ss;
        private float* sdr;                         // fbW * fbH * {top rgb, bottom rgb}: page-locked memory of the library
        private readonly bool deviceColors;
        private byte* color16;                      // DeviceChexelColors: {color_16 of top | of bottom << 4} per chexel
        private readonly DeviceAnsiTerminalRenderer ansi;
        private byte* ansiBuf;
        private ulong ansiCap, ansiLen;
        private readonly bool ansiDelta;            // HipRaytraceOptions.DeviceAnsiDelta: delta streams, on the delta state the context shares with the ray-traced frames
        private readonly int ansiMergeGap;
        private readonly bool ansiRgb;              // HipRaytraceOptions.AnsiTrueColor: the 24-bit colour forms
        private readonly int ansiTolerance;
        private readonly bool ansiQuad;             // HipRaytraceOptions.QuadrantGlyphs: the quadrant-glyph forms (superSample even)
        private readonly int ansiMinContrast;
        private readonly bool sixel, sixelDither, sixelDelta;   // HipRaytraceOptions.SixelGraphics: the sixel forms in place of every stream form
        private bool sixelBufOwned;                 // ... ansiBuf is pageable memory of this wrapper (Marshal), not the library's page-locked memory
        private readonly bool sixelPalette, sixelHold;   // HipRaytraceOptions.SixelAdaptivePalette / SixelHoldPalette: ycge_video_blit_sixel_palette
        private bool sixelRebuild;                  // ... the next frame builds its palette whatever sixelHold says

        /// <summary>sharedContext: the context of the raytrace wrapper of the same console, whose geometry must be fb's and superSample's
        /// (IntPtr.Zero: a context of this wrapper's own).</summary>
        public HipVideoWrapper(Framebuffer fb, IFrameReader reader, int superSample, bool requestRGBA, HipRaytraceOptions options = null, IntPtr sharedContext = default)
        {
            this.reader = reader ?? throw new ArgumentNullException(nameof(reader));
            useRGBA = requestRGBA;
            fbW = fb.Width; fbH = fb.Height; ss = Math.Max(1, superSample);         // VideoRenderer.cs:33-37
            ansi = options != null && options.DeviceAnsiStream ? options.AnsiPresenter ?? throw new ArgumentException("DeviceAnsiStream needs an AnsiPresenter") : null;
            ansiDelta = ansi != null && options.DeviceAnsiDelta; ansiMergeGap = options != null ? options.AnsiMergeGap : 3;
            ansiRgb = ansi != null && options.AnsiTrueColor; ansiTolerance = options != null ? options.AnsiRgbTolerance : 0;
            ansiQuad = ansi != null && options.QuadrantGlyphs; ansiMinContrast = options != null ? options.QuadrantMinContrast : 0;
            if (ansiQuad && (ss & 1) != 0) throw new ArgumentException("QuadrantGlyphs needs an even superSample");
            ansiRgb |= ansiQuad;                    // (the quadrant streams are 24-bit ones: their bound is the 24-bit bound)
            sixel = ansi != null && options.SixelGraphics; sixelDither = sixel && options.SixelDither; sixelDelta = sixel && options.SixelDelta;
            if (sixel && (options.DeviceAnsiDelta || options.QuadrantGlyphs)) throw new ArgumentException("SixelGraphics has no ANSI delta or quadrant form");
            sixelPalette = sixel && options.SixelAdaptivePalette; sixelHold = sixelPalette && options.SixelHoldPalette;
            if (sixelPalette && (sixelDither || sixelDelta)) throw new ArgumentException("SixelAdaptivePalette has no dither and no delta form");
            deviceColors = options != null && options.DeviceChexelColors;
            if (sharedContext != IntPtr.Zero)
            {
                // The raytrace wrapper made (or last resized) this context for the same framebuffer and superSample: no ycge_resize here, which
                // would drop the TAA history (RaytraceRenderer.cs:137) of the frames the user comes back to.  Resize() below is the seam's own.
                ctx = sharedContext;
            }
            else
            {
                var cfg = new YConfig();
                Ycge.Check(IntPtr.Zero, Ycge.ycge_config_default(ref cfg));
                cfg.FbWidth = fbW; cfg.FbHeight = fbH; cfg.SuperSample = ss;
                if (options?.Devices != null && options.Devices.Length > 0) cfg.Device = options.Devices[0];      // (a blit runs on one device)
                Ycge.Check(IntPtr.Zero, Ycge.ycge_create(ref cfg, out ctx));
                ownsContext = true;
            }
            AllocFrame();
            if (ansi != null) ansi.Source = () => LastAnsiFrame;
        }

        public ReadOnlySpan<byte> LastAnsiFrame => ansiBuf == null ? ReadOnlySpan<byte>.Empty : new ReadOnlySpan<byte>(ansiBuf, checked((int)ansiLen));

        private void AllocFrame()
        {
            FreeFrame();
            Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer((UIntPtr)((ulong)fbW * (ulong)fbH * 6 * sizeof(float)), out IntPtr p));
            sdr = (float*)p;
            if (deviceColors) { Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer((UIntPtr)((ulong)fbW * (ulong)fbH), out IntPtr c)); color16 = (byte*)c; }
        }

        private void FreeFrame()
        {
            if (sdr != null) { Ycge.ycge_free_host_buffer((IntPtr)sdr); sdr = null; }
            if (color16 != null) { Ycge.ycge_free_host_buffer((IntPtr)color16); color16 = null; }
        }

        public void SetCamera(Vec3 pos, float yaw, float pitch) { /* no-op for video (RaytraceEntity.cs:41) */ }
        public void SetFov(float fovDeg) { /* no-op for video (RaytraceEntity.cs:42) */ }

        public void Resize(Framebuffer fb, int superSample)
        {
            fbW = fb.Width; fbH = fb.Height; ss = Math.Max(1, superSample);
            if (ansiQuad && (ss & 1) != 0) throw new ArgumentException("QuadrantGlyphs needs an even superSample");
            Ycge.Check(ctx, Ycge.ycge_resize(ctx, fbW, fbH, ss));
            AllocFrame();
        }

        public void TryFlipAndBlit(Framebuffer fb)
        {
            if (fb == null) throw new ArgumentNullException(nameof(fb));
            IntPtr frame = reader.GetCurrentFramePtr();                        // VideoRenderer.cs:71-73, 83
            int srcW = reader.Width, srcH = reader.Height, bpp = useRGBA ? 4 : 3;
            if (sixel) { BlitSixel(fb, frame, srcW, srcH, bpp); return; }
            if (ansi != null)
            {
                int cw = ansi.consoleWidth, ch = ansi.consoleHeight;
                UIntPtr bound;
                if (ansiRgb) Ycge.Check(ctx, Ycge.ycge_ansi_rgb_stream_bound(cw, ch, out bound));
                else Ycge.Check(ctx, Ycge.ycge_ansi_stream_bound(cw, ch, out bound));
                if ((ulong)bound > ansiCap)
                {
                    if (ansiBuf != null) { Ycge.ycge_free_host_buffer((IntPtr)ansiBuf); ansiBuf = null; ansiCap = ansiLen = 0; }
                    Ycge.Check(ctx, Ycge.ycge_alloc_host_buffer(bound, out IntPtr p));
                    ansiBuf = (byte*)p; ansiCap = (ulong)bound;
                }
                HipConsoleLayers.Set(ctx, ansi.FrameBuffers, fb);               // (the presenter's other framebuffers, composed on the device)
                UIntPtr len;
                if (ansiQuad && ansiDelta)
                    Ycge.Check(ctx, Ycge.ycge_video_blit_ansi_quad_delta(ctx, frame, srcW, srcH, bpp, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg,
                                                                         ansi.ClearPending ? 1 : 0, ansiMergeGap, ansiTolerance, 0, ansiMinContrast, ansiBuf, (UIntPtr)ansiCap, &len,
                                                                         null, null));
                else if (ansiQuad)
                    Ycge.Check(ctx, Ycge.ycge_video_blit_ansi_quad(ctx, frame, srcW, srcH, bpp, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg,
                                                                   ansi.ClearPending ? 1 : 0, ansiMinContrast, ansiBuf, (UIntPtr)ansiCap, &len, null));
                else if (ansiRgb && ansiDelta)
                    Ycge.Check(ctx, Ycge.ycge_video_blit_ansi_rgb_delta(ctx, frame, srcW, srcH, bpp, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg,
                                                                        ansi.ClearPending ? 1 : 0, ansiMergeGap, ansiTolerance, 0, ansiBuf, (UIntPtr)ansiCap, &len, null, null));
                else if (ansiRgb)
                    Ycge.Check(ctx, Ycge.ycge_video_blit_ansi_rgb(ctx, frame, srcW, srcH, bpp, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg,
                                                                  ansi.ClearPending ? 1 : 0, ansiBuf, (UIntPtr)ansiCap, &len, null));
                else if (ansiDelta)
                    Ycge.Check(ctx, Ycge.ycge_video_blit_ansi_delta(ctx, frame, srcW, srcH, bpp, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg,
                                                                    ansi.ClearPending ? 1 : 0, ansiMergeGap, 0, ansiBuf, (UIntPtr)ansiCap, &len, null, null));
                else
                    Ycge.Check(ctx, Ycge.ycge_video_blit_ansi(ctx, frame, srcW, srcH, bpp, cw, ch, fb.ViewportX, fb.ViewportY, (int)ansi.DefaultFg, (int)ansi.DefaultBg,
                                                              ansi.ClearPending ? 1 : 0, ansiBuf, (UIntPtr)ansiCap, &len, null));
                ansiLen = (ulong)len;
                ansi.ClearPending = false;
                return;                                                        // (the presenter writes the stream: the framebuffer is not walked)
            }
            Ycge.Check(ctx, Ycge.ycge_video_blit(ctx, frame, srcW, srcH, bpp, sdr, deviceColors ? color16 : null, null, null));
            for (int cy = 0; cy < fbH; cy++)
                for (int cx = 0; cx < fbW; cx++)
                {
                    float* c = sdr + ((long)cx + (long)cy * fbW) * 6;          // {topAvg, botAvg} of VideoRenderer.cs:127-128
                    if (deviceColors)
                    {
                        byte b = color16[(long)cx + (long)cy * fbW];
                        fb.SetChexel(cx, cy, new Chexel('▀', new ChexelColor((ConsoleColor)(b & 15), new Vec3(c[0], c[1], c[2])),
                                                             new ChexelColor((ConsoleColor)(b >> 4), new Vec3(c[3], c[4], c[5]))));
                    }
                    else fb.SetChexel(cx, cy, new Chexel('▀', new Vec3(c[0], c[1], c[2]), new Vec3(c[3], c[4], c[5])));      // :130, :144
                }
        }

        /// <summary>SixelHoldPalette: the next frame builds a new palette from its picture (a cut in the film, every N frames)</summary>
        public void SixelRebuildPalette() { sixelRebuild = true; }

        // SixelGraphics: the frame as the sixel stream of the blit's hi-res samples at the framebuffer's viewport; the buffer is pageable memory of
        // the bound's size, as HipRaytraceWrapper's
        private void BlitSixel(Framebuffer fb, IntPtr frame, int srcW, int srcH, int bpp)
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
                Ycge.Check(ctx, Ycge.ycge_video_blit_sixel_palette(ctx, frame, srcW, srcH, bpp, fb.ViewportX, fb.ViewportY, ansi.ClearPending ? 1 : 0, sixelHold && !sixelRebuild ? 1 : 0,
                                                                   ansiBuf, (UIntPtr)ansiCap, &len, null, null, null));
                sixelRebuild = false;
            }
            else if (sixelDelta)
                Ycge.Check(ctx, Ycge.ycge_video_blit_sixel_delta(ctx, frame, srcW, srcH, bpp, fb.ViewportX, fb.ViewportY, ansi.ClearPending ? 1 : 0, 0, sixelDither ? 1 : 0, ansiBuf,
                                                                 (UIntPtr)ansiCap, &len, null, null));
            else
                Ycge.Check(ctx, Ycge.ycge_video_blit_sixel(ctx, frame, srcW, srcH, bpp, fb.ViewportX, fb.ViewportY, ansi.ClearPending ? 1 : 0, sixelDither ? 1 : 0, ansiBuf,
                                                           (UIntPtr)ansiCap, &len, null));
            ansiLen = (ulong)len;
            ansi.ClearPending = false;
        }

        private void FreeAnsiBuf()
        {
            if (ansiBuf == null) return;
            if (sixelBufOwned) System.Runtime.InteropServices.Marshal.FreeHGlobal((IntPtr)ansiBuf); else Ycge.ycge_free_host_buffer((IntPtr)ansiBuf);
            ansiBuf = null; sixelBufOwned = false; ansiCap = ansiLen = 0;
        }

        public void Dispose()
        {
            if (ownsContext && ctx != IntPtr.Zero) Ycge.ycge_destroy(ctx);
            ctx = IntPtr.Zero;
            FreeFrame();
            FreeAnsiBuf();
            reader?.Dispose();                                                 // VideoRenderer.Dispose (:150-153)
        }
    }
}
