// YcgeConsole.cs - ycge_chexel and ycge_console_layer (include/ycge.h): the console's other framebuffers for Ycge.ycge_console_set_layers,
// and HipConsoleLayers, which flattens a presenter's framebuffer list into them.  YChexel is 28 bytes, 4-byte aligned: the UTF-16 code
// unit, two bytes of padding, ForegroundColor.color_f32 and BackgroundColor.color_f32.  YConsoleLayer: four ints and the cells' pointer.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;
using ConsoleGame.Renderer;

namespace ConsoleGame.RayTracing.Native
{
    [StructLayout(LayoutKind.Sequential)]
    public struct YChexel             // ycge_chexel
    {
        public ushort Ch;             // Chexel.Char
        public ushort Pad;
        public YVec3 Fg;              // ForegroundColor.color_f32
        public YVec3 Bg;              // BackgroundColor.color_f32
    }

    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct YConsoleLayer   // ycge_console_layer
    {
        public int X, Y, W, H;        // Framebuffer.ViewportX, ViewportY, Width, Height
        public YChexel* Cells;        // row by row: cell (x, y) at y * W + x
    }

    /// <summary>ANSITerminalRenderer's frameBuffers list (ANSITerminalRenderer.cs:56-65) as the device streams take it: every framebuffer but
    /// the wrapper's own goes up as a layer, in list order, and raytrace_at is the index of the wrapper's own framebuffer in the list (a
    /// framebuffer the presenter does not hold is drawn on top).  Chexel[x, y] is transposed to rows.  The library copies the cells.</summary>
    public static unsafe class HipConsoleLayers
    {
        public const int MaxLayers = 16;          // YCGE_CONSOLE_MAX_LAYERS

        public static void Set(IntPtr ctx, IReadOnlyList<Framebuffer> frameBuffers, Framebuffer own)
        {
            var others = new List<Framebuffer>();
            int raytraceAt = -1;
            foreach (Framebuffer fb in frameBuffers)
            {
                if (ReferenceEquals(fb, own)) { if (raytraceAt < 0) raytraceAt = others.Count; }
                else if (fb.Width > 0 && fb.Height > 0) others.Add(fb);
            }
            if (raytraceAt < 0) raytraceAt = others.Count;
            if (others.Count > MaxLayers) throw new InvalidOperationException("at most 16 framebuffers beside the raytrace one (YCGE_CONSOLE_MAX_LAYERS)");
            if (others.Count == 0) { Ycge.Check(ctx, Ycge.ycge_console_set_layers(ctx, null, 0, 0)); return; }
            long total = 0;
            foreach (Framebuffer fb in others) total += (long)fb.Width * fb.Height;
            var cells = new YChexel[total];
            var layers = new YConsoleLayer[others.Count];
            fixed (YChexel* c = cells) fixed (YConsoleLayer* l = layers)
            {
                long at = 0;
                for (int k = 0; k < others.Count; k++)
                {
                    Framebuffer fb = others[k];
                    l[k] = new YConsoleLayer { X = fb.ViewportX, Y = fb.ViewportY, W = fb.Width, H = fb.Height, Cells = c + at };
                    for (int y = 0; y < fb.Height; y++)
                        for (int x = 0; x < fb.Width; x++)
                        {
                            Chexel s = fb.GetChexel(x, y);
                            c[at++] = new YChexel { Ch = s.Char, Fg = new YVec3(s.ForegroundColor.color_f32), Bg = new YVec3(s.BackgroundColor.color_f32) };
                        }
                }
                Ycge.Check(ctx, Ycge.ycge_console_set_layers(ctx, l, others.Count, raytraceAt));
            }
        }
    }
}
