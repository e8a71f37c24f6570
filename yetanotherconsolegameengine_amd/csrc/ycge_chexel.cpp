// ycge_chexel.cpp - the presenters' colour maps on the device (ycge_render_frame_chexels, ycge_render_frame_async_chexels; kernel:
// ycge_chexel.hip).
//
// A frame of these calls is ycge_render_frame's (or ycge_render_frame_async_sdr's) with the post stage, plus one launch behind the tonemap
// on the same stream that turns the SDR array into the bytes the caller asked for, and their read-back.  What the caller asked for is
// the entry point's FrameOutputs (ycge_ctx.h), handed down to run_post and from there to this file: an entry point that asks for no
// chexels hands down a value that names none, and issues no extra launch, copy or event.
//
// LinearToSrgb8 (ANSITerminalRenderer.cs:287-296 = OpenGLTerminalRenderer.cs:390-400) is a monotone step function of its input: the
// host finds its 255 steps ONCE with the C library's double pow - the function Math.Pow calls - and the kernel counts thresholds.
// One table for binary32 inputs (the channels), one for binary64 (the luminance, a genuine double).
#include "ycge_ctx.h"

#include <cmath>

namespace {

// LinearToSrgb8 as the reference writes it: clamp, the sRGB curve in double, Math.Round (half to even: nearbyint in the default
// rounding mode), the int clamp (NaN: (int)NaN is int.MinValue before .NET 9 and 0 from it - both clamp to 0)
int linear_to_srgb8(double c)
{
    if (c < 0.0) c = 0.0;
    if (c > 1.0) c = 1.0;
    const double s = c <= 0.0031308 ? 12.92 * c : 1.055 * std::pow(c, 1.0 / 2.4) - 0.055;
    const double r = std::nearbyint(s * 255.0);
    if (!(r >= 0.0)) return 0;
    return r > 255.0 ? 255 : (int)r;
}

// the thresholds: entry k - 1 is the smallest non-negative value of the type whose byte is >= k (binary search over the bit patterns,
// which order non-negative floats); entry 255 is a NaN nobody compares with
struct SrgbTables {
    float t32[256];
    double t64[256];
    SrgbTables()
    {
        for (int k = 1; k <= 255; k++) {
            uint32_t lo = 0, hi = 0x3f800000u;                 // byte(1.0f) = 255 >= k
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                float x; std::memcpy(&x, &mid, 4);
                if (linear_to_srgb8((double)x) >= k) hi = mid; else lo = mid + 1;
            }
            std::memcpy(&t32[k - 1], &lo, 4);
            uint64_t lo8 = 0, hi8 = 0x3ff0000000000000ull;
            while (lo8 < hi8) {
                const uint64_t mid = lo8 + (hi8 - lo8) / 2;
                double x; std::memcpy(&x, &mid, 8);
                if (linear_to_srgb8(x) >= k) hi8 = mid; else lo8 = mid + 1;
            }
            std::memcpy(&t64[k - 1], &lo8, 8);
        }
        t32[255] = std::nanf("");
        t64[255] = std::nan("");
    }
};

const SrgbTables &srgb_tables()
{
    static const SrgbTables t;            // (thread-safe initialisation; no heap)
    return t;
}

// offsets of the three outputs in one device buffer of n chexels (aligned for the kernel's 2- and 4-byte stores)
struct ChexelLayout {
    size_t n, c16, ansi, rgba, total;
    explicit ChexelLayout(size_t n_) : n(n_)
    {
        c16 = 0;
        ansi = (n + 255) & ~(size_t)255;
        rgba = ansi + ((2 * n + 255) & ~(size_t)255);
        total = rgba + 8 * n;
    }
};

// where the frame's colour plane of asked's stream lies (AnsiPlan::frame_in_held): chexel_encode writes it there - a _delta call's where the
// next call finds it; 24-bit: a keyframe's plane is the next `shown`, a delta's write kernel fills that - and the stream kernels read it there
uint8_t *ansi_frame_plane(ChexelState &X, const FrameOutputs &asked,const ChexelLayout &L, bool second)
{
    if (asked.plan.frame_in_held) return X.delta_held[1 - X.delta_prev].p;
    return X.out[second ? 1 : 0].p + (asked.ansi->rgb ? L.rgba : L.ansi);
}

} // namespace

namespace ycge_host {

int check_quadrant_call(ycge_ctx *c, const char *fn, int32_t min_contrast)
{
    if (c->ss < 2 || (c->ss & 1))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: super_sample %d (the quadrants halve a chexel's columns: it must be even)", fn, c->ss);
    if (min_contrast < 0 || min_contrast > 255) return c->fail(YCGE_ERR_INVALID_ARG, "%s: min_contrast %d (0..255)", fn, min_contrast);
    return YCGE_OK;
}

int ensure_tables(ycge_ctx *c, ChexelState &X)
{
    if (X.tables.p) return YCGE_OK;
    const SrgbTables &t = srgb_tables();
    uint8_t host[3072];
    std::memcpy(host, t.t32, 1024);
    std::memcpy(host + 1024, t.t64, 2048);
    HIP_TRY(c, X.tables.alloc(sizeof host));
    const hipError_t e = hipMemcpy(X.tables.p, host, sizeof host, hipMemcpyHostToDevice);
    if (e != hipSuccess) { X.tables.release(); HIP_TRY(c, e); }
    return YCGE_OK;
}

int chexel_encode(ycge_ctx *c, hipStream_t stream, const FrameOutputs &asked, const float *d_sdr, bool second)
{
    if (asked.pixels) return sixel_encode(c, stream, asked);                             // (the sixel presenter: ycge_sixel.cpp)
    ChexelState *X = &c->chexels;
    uint8_t *const *dst = asked.chexels;
    const bool ansi = asked.ansi != nullptr;                                             // (ycge_render_frame_ansi: the pairs stay on the device)
    const bool quad = asked.quad || (ansi && asked.ansi->quad);                          // (the quadrant calls: the fit's planes for the encoder's)
    if (!dst[0] && !dst[1] && !dst[2] && !ansi && !quad) return YCGE_OK;                 // (the SDR alone: nothing to encode)
    // (frames in flight: the stream buffers are one set per context - this frame's encode .. deliver follows the deliver of the frame before)
    if (ansi && X->flight_pending && X->flight_stream != stream) HIP_TRY(c, hipStreamWaitEvent(stream, X->flight_ev, 0));
    const ChexelLayout L((size_t)c->fbW * c->fbH);
    DevBuf<uint8_t> &out = X->out[second ? 1 : 0];
    if (out.cap < L.total) HIP_TRY(c, out.alloc(L.total));
    if (dst[1] || dst[2] || ansi || quad) { const int rc = ensure_tables(c, *X); if (rc != YCGE_OK) return rc; }
    if (quad) {
        // k_tonemap_quadrants on the buffer and exposure state the tonemap in front of this read, then the fit: the glyph plane, and the RGBA
        // plane where the encoder's lies.  The held planes of a _quad_delta call are the composite's (ycge_ansi.cpp), so nothing moves here.
        // A video blit's sub-cell colours are there already (k_video_blit_quadrants, no tone map): the fit alone.
        if (X->quad_sdr.cap < 12 * L.n) {
            if (asked.quad_colours_ready) return c->fail(YCGE_ERR_INTERNAL, "chexel_encode: the sub-cell colours of %zu chexels are not on the device", L.n);
            HIP_TRY(c, X->quad_sdr.alloc(12 * L.n));
        }
        if (X->quad_glyphs.cap < L.n) HIP_TRY(c, X->quad_glyphs.alloc(L.n));
        int e = 0;
        if (!asked.quad_colours_ready) {
            e = ycge_launch_tonemap_quadrants(c->denoised, c->hiW, c->fbW, c->fbH, c->ss, 2.2f, 2.0f, 0.0f, c->tone_state.p, X->quad_sdr.p, stream);
            if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_tonemap_quadrants launch failed: %s", hipGetErrorString((hipError_t)e));
        }
        e = ycge_launch_quadrant_fit(X->quad_sdr.p, c->fbW, c->fbH, X->tables.p, asked.quad ? asked.quad->min_contrast : asked.ansi->min_contrast, X->quad_glyphs.p,
                                     out.p + L.rgba, c->compute_units, stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_fit_quadrants launch failed: %s", hipGetErrorString((hipError_t)e));
        return YCGE_OK;
    }
    const bool rgb = ansi && asked.ansi->rgb;                                            // (a 24-bit stream: the RGBA plane stays on the device instead)
    uint8_t *pairs = out.p + L.ansi, *rgba = out.p + L.rgba;
    if (ansi) (rgb ? rgba : pairs) = ansi_frame_plane(*X, asked, L, second);
    const int e = ycge_launch_chexels(d_sdr, c->fbW, c->fbH, X->tables.p, dst[0] ? out.p + L.c16 : nullptr, dst[1] || (ansi && !rgb) ? pairs : nullptr,
                                      dst[2] || rgb ? rgba : nullptr, c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_encode_chexels launch failed: %s", hipGetErrorString((hipError_t)e));
    return YCGE_OK;
}

// ycge_render_frame_quadrants' copies: the sub-cell colours, the glyph plane, the fitted RGBA plane - pageable destinations staged one
// behind the other, as below
static int quadrants_read_back(ycge_ctx *c, hipStream_t stream, FrameOutputs &out, bool second)
{
    ChexelState *X = &c->chexels;
    const ChexelLayout L((size_t)c->fbW * c->fbH);
    void *dst[3] = {out.quad->sdr, out.quad->glyphs, out.quad->rgba};
    const void *src[3] = {X->quad_sdr.p, X->quad_glyphs.p, X->out[second ? 1 : 0].p + L.rgba};
    const size_t bytes[3] = {48 * L.n, 2 * L.n, 8 * L.n}, off[3] = {0, 48 * L.n, 56 * L.n};          // (48 n and 56 n: multiples of 8)
    size_t staged = 0;
    for (int k = 0; k < 3; k++)
        if (dst[k] && !host_memory_is_page_locked(dst[k], bytes[k])) staged = off[k] + bytes[k];
    HIP_TRY(c, X->stage.reserve(staged));
    for (int k = 0; k < 3; k++) {
        if (!dst[k]) continue;
        void *target = dst[k];
        if (!host_memory_is_page_locked(dst[k], bytes[k])) target = out.redirect(dst[k], X->stage.data() + off[k], bytes[k]);
        HIP_TRY(c, hipMemcpyAsync(target, src[k], bytes[k], hipMemcpyDeviceToHost, stream));
    }
    return YCGE_OK;
}

int chexel_read_back(ycge_ctx *c, hipStream_t stream, FrameOutputs &out, bool second)
{
    ChexelState *X = &c->chexels;
    uint8_t *const *dst = out.chexels;
    if (out.pixels) return sixel_read_back(c, stream, out);
    if (out.quad) return quadrants_read_back(c, stream, out, second);
    if (!dst[0] && !dst[1] && !dst[2] && !out.ansi) return YCGE_OK;
    const ChexelLayout L((size_t)c->fbW * c->fbH);
    const size_t off[3] = {L.c16, L.ansi, L.rgba}, bytes[3] = {L.n, 2 * L.n, 8 * L.n};
    const uint8_t *src = X->out[second ? 1 : 0].p;
    size_t staged = 0;
    for (int k = 0; k < 3; k++)
        if (dst[k] && !host_memory_is_page_locked(dst[k], bytes[k])) staged = off[k] + bytes[k];
    HIP_TRY(c, X->stage.reserve(staged));
    for (int k = 0; k < 3; k++) {
        if (!dst[k]) continue;
        uint8_t *target = dst[k];
        if (!host_memory_is_page_locked(dst[k], bytes[k]))             // (synchronous calls only: the frames in flight refuse pageable arrays up front)
            target = out.redirect(dst[k], X->stage.data() + off[k], bytes[k]);
        HIP_TRY(c, hipMemcpyAsync(target, src + off[k], bytes[k], hipMemcpyDeviceToHost, stream));
    }
    if (!out.ansi) return YCGE_OK;
    // (ycge_ansi.cpp: the escape stream and its length from the pairs - 24-bit: the RGBA plane - where chexel_encode put them)
    return ansi_enqueue(c, stream, out, ansi_frame_plane(*X, out, L, second));
}

} // namespace ycge_host

namespace {

int check_chexel_call(ycge_ctx *c, const char *fn, const FrameOutputs &out)
{
    if (!out.sdr && !out.chexels[0] && !out.chexels[1] && !out.chexels[2])
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: every destination is NULL (ask for at least one of sdr, color16, ansi, rgba)", fn);
    return YCGE_OK;
}

} // namespace

// =========================================================================== C-ABI
extern "C" {

int ycge_render_frame_chexels(ycge_ctx *c, float *out_top_bottom_sdr, uint8_t *out_color16, uint8_t *out_ansi, uint8_t *out_rgba, ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    FrameOutputs out(out_top_bottom_sdr, out_color16, out_ansi, out_rgba);
    int rc = check_chexel_call(c, "ycge_render_frame_chexels", out);
    if (rc == YCGE_OK) rc = check_post_frame(c);
    return rc == YCGE_OK ? render_frame_sync(c, &out, st) : rc;
}
catch (...) { return ycge_host::abi_catch(c); }

// The quadrant-glyph planes (the contract: include/ycge.h): ycge_render_frame_chexels' frame with k_tonemap_quadrants and k_fit_quadrants
// behind the tonemap for the encoder
int ycge_render_frame_quadrants(ycge_ctx *c, float *out_top_bottom_sdr, float *out_quad_sdr, uint16_t *out_glyphs, uint8_t *out_rgba, int32_t min_contrast,
                                ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_render_frame_quadrants";
    if (!out_top_bottom_sdr && !out_quad_sdr && !out_glyphs && !out_rgba)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: every destination is NULL (ask for at least one of sdr, quad_sdr, glyphs, rgba)", fn);
    int rc = check_quadrant_call(c, fn, min_contrast);
    if (rc == YCGE_OK) rc = check_post_frame(c);
    if (rc != YCGE_OK) return rc;
    const FrameOutputs::Quadrants q{out_quad_sdr, out_glyphs, out_rgba, min_contrast};
    FrameOutputs out(out_top_bottom_sdr);
    if (out_quad_sdr || out_glyphs || out_rgba) out.quad = &q;          // (the SDR alone: ycge_render_frame's frame)
    return render_frame_sync(c, &out, st);
}
catch (...) { return ycge_host::abi_catch(c); }

// The sixel presenter (the contract: include/ycge.h; the bodies: ycge_sixel.cpp): the bound, the host encoder, the planes of a frame's
// hi-res samples, their sixel stream, and the two test hooks - the pixel stage and the encoder's kernels alone
int ycge_sixel_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes)
try {
    return sixel_stream_bound(px_w, px_h, bytes);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_sixel_encode_host(const uint8_t *index, int32_t px_w, int32_t px_h, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, uint8_t *out_stream,
                           size_t capacity, size_t *out_len)
try {
    return sixel_encode_host(index, px_w, px_h, viewport_x, viewport_y, clear_screen, out_stream, capacity, out_len);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_pixels(ycge_ctx *c, float *out_top_bottom_sdr, uint8_t *out_rgba, uint8_t *out_index, int32_t dither, ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_frame_pixels(c, out_top_bottom_sdr, out_rgba, out_index, dither, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_sixel(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t dither, uint8_t *out_stream, size_t capacity,
                            size_t *out_len, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_frame_stream(c, viewport_x, viewport_y, clear_screen, dither, out_stream, capacity, out_len, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_pixels(ycge_ctx *c, const float *hdr, int32_t fbW, int32_t fbH, int32_t ss, float exposure, int32_t dither, uint8_t *out_rgba, uint8_t *out_index)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_test_pixels(c, hdr, fbW, fbH, ss, exposure, dither, out_rgba, out_index);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_sixel_stream(ycge_ctx *c, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_test_stream(c, index, W, H, vx, vy, clear, out, capacity, out_len);
}
catch (...) { return ycge_host::abi_catch(c); }

// The delta and Video mode forms of the sixel presenter (the bodies: ycge_sixel.cpp, ycge_video.cpp) and their two hooks
int ycge_sixel_encode_delta_host(const uint8_t *prev_index, const uint8_t *index, int32_t px_w, int32_t px_h, int32_t viewport_x, int32_t viewport_y, uint8_t *out_stream,
                                 size_t capacity, size_t *out_len, uint32_t *out_info)
try {
    return sixel_encode_delta_host(prev_index, index, px_w, px_h, viewport_x, viewport_y, out_stream, capacity, out_len, out_info);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_sixel_delta(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream,
                                  size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_frame_stream_delta(c, viewport_x, viewport_y, clear_screen, keyframe, dither, out_stream, capacity, out_len, out_info, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, float *out_top_bottom_sdr, uint8_t *out_rgba,
                           uint8_t *out_index, int32_t dither)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_video_pixels(c, frame, src_w, src_h, bytes_per_pixel, out_top_bottom_sdr, out_rgba, out_index, dither);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_sixel(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t viewport_x, int32_t viewport_y,
                          int32_t clear_screen, int32_t dither, uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_video_stream(c, "ycge_video_blit_sixel", frame, src_w, src_h, bytes_per_pixel, viewport_x, viewport_y, clear_screen, -1, dither, out_stream, capacity,
                              out_len, nullptr, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_sixel_delta(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t viewport_x, int32_t viewport_y,
                                int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                                float *out_top_bottom_sdr)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_video_stream(c, "ycge_video_blit_sixel_delta", frame, src_w, src_h, bytes_per_pixel, viewport_x, viewport_y, clear_screen, keyframe != 0 ? 1 : 0, dither,
                              out_stream, capacity, out_len, out_info, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_video_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t fbW, int32_t fbH, int32_t ss, int32_t dither,
                           uint8_t *out_rgba, uint8_t *out_index)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_test_video_pixels(c, frame, src_w, src_h, bytes_per_pixel, fbW, fbH, ss, dither, out_rgba, out_index);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_sixel_delta_stream(ycge_ctx *c, const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity,
                                 size_t *out_len, uint32_t *out_info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_test_delta_stream(c, prev, index, W, H, vx, vy, out, capacity, out_len, out_info);
}
catch (...) { return ycge_host::abi_catch(c); }

// The adaptive sixel palette (the bodies: ycge_sixel.cpp; the plain C++: ycge_sixel_host.cpp) and its two hooks
int ycge_sixel_palette_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes)
try {
    return sixel_palette_stream_bound(px_w, px_h, bytes);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_sixel_palette_host(const uint8_t *rgba, int32_t px_w, int32_t px_h, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count)
try {
    return sixel_palette_host(rgba, px_w, px_h, out_index, out_palette, out_pct, out_count);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_sixel_encode_palette_host(const uint8_t *index, const uint8_t *pct, int32_t count, int32_t px_w, int32_t px_h, int32_t viewport_x, int32_t viewport_y,
                                   int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len)
try {
    return sixel_encode_palette_host(index, pct, count, px_w, px_h, viewport_x, viewport_y, clear_screen, out_stream, capacity, out_len);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_sixel_palette(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t hold, uint8_t *out_stream, size_t capacity,
                                    size_t *out_len, uint8_t *out_palette, int32_t *out_count, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_frame_palette(c, "ycge_render_frame_sixel_palette", true, viewport_x, viewport_y, clear_screen, hold, out_stream, capacity, out_len, nullptr, nullptr,
                               out_palette, out_count, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_pixels_palette(ycge_ctx *c, float *out_top_bottom_sdr, uint8_t *out_rgba, uint8_t *out_index, int32_t hold, uint8_t *out_palette, int32_t *out_count,
                                     ycge_frame_stats *st)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_frame_palette(c, "ycge_render_frame_pixels_palette", false, 0, 0, 0, hold, nullptr, 0, nullptr, out_rgba, out_index, out_palette, out_count,
                               out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_sixel_palette(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t viewport_x, int32_t viewport_y,
                                  int32_t clear_screen, int32_t hold, uint8_t *out_stream, size_t capacity, size_t *out_len, uint8_t *out_palette, int32_t *out_count,
                                  float *out_top_bottom_sdr)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_video_palette(c, "ycge_video_blit_sixel_palette", true, frame, src_w, src_h, bytes_per_pixel, viewport_x, viewport_y, clear_screen, hold, out_stream,
                               capacity, out_len, nullptr, nullptr, out_palette, out_count, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_pixels_palette(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, float *out_top_bottom_sdr, uint8_t *out_rgba,
                                   uint8_t *out_index, int32_t hold, uint8_t *out_palette, int32_t *out_count)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_video_palette(c, "ycge_video_blit_pixels_palette", false, frame, src_w, src_h, bytes_per_pixel, 0, 0, 0, hold, nullptr, 0, nullptr, out_rgba, out_index,
                               out_palette, out_count, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_sixel_palette(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t hold, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct,
                            int32_t *out_count)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_test_palette(c, rgba, W, H, hold, out_index, out_palette, out_pct, out_count);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_sixel_palette_stream(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, int32_t hold, uint8_t *out,
                                   size_t capacity, size_t *out_len)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return sixel_test_palette_stream(c, rgba, W, H, vx, vy, clear, hold, out, capacity, out_len);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_async_chexels(ycge_ctx *c, float *out_top_bottom_sdr, uint8_t *out_color16, uint8_t *out_ansi, uint8_t *out_rgba)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    FrameOutputs out(out_top_bottom_sdr, out_color16, out_ansi, out_rgba);
    int rc = check_chexel_call(c, "ycge_render_frame_async_chexels", out);
    if (rc == YCGE_OK) rc = check_post_frame(c);
    if (rc != YCGE_OK) return rc;
    const size_t n = (size_t)c->fbW * c->fbH;
    const void *dst[4] = {out_top_bottom_sdr, out_color16, out_ansi, out_rgba};
    const size_t bytes[4] = {n * 6 * sizeof(float), n, 2 * n, 8 * n};
    const char *names[4] = {"sdr", "color16", "ansi", "rgba"};
    for (int k = 0; k < 4; k++)
        if (dst[k] && !host_memory_is_page_locked(dst[k], bytes[k]))
            return c->fail(YCGE_ERR_INVALID_ARG, "ycge_render_frame_async_chexels fills its arrays while the caller runs on: %s must be page-locked memory "
                                                 "(ycge_alloc_host_buffer, or whole pages registered with ycge_pin_host_buffer)", names[k]);
    return render_frame_in_flight(c, &out);
}
catch (...) { return ycge_host::abi_catch(c); }

// Video mode (ycge_video.cpp): VideoRenderer.TryFlipAndBlit of the frame the host's IFrameReader shows, into the destinations of
// ycge_render_frame_chexels.  Upload and k_video_blit, then this file's encode and read-back on the same stream, then one synchronisation.
int ycge_video_blit(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, float *out_top_bottom_sdr, uint8_t *out_color16,
                    uint8_t *out_ansi, uint8_t *out_rgba)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_video_blit";
    int rc = video_check_frame(c, fn, frame, src_w, src_h, bytes_per_pixel);
    FrameOutputs out(out_top_bottom_sdr, out_color16, out_ansi, out_rgba);
    if (rc == YCGE_OK) rc = check_chexel_call(c, fn, out);
    if (rc != YCGE_OK) return rc;
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const float *d_sdr = nullptr;
    rc = video_enqueue(c, c->stream, frame, src_w, src_h, bytes_per_pixel, c->fbW, c->fbH, c->ss, &d_sdr);
    if (rc == YCGE_OK) rc = chexel_encode(c, c->stream, out, d_sdr, false);
    if (rc == YCGE_OK) rc = video_read_sdr(c, c->stream, d_sdr, out);
    if (rc == YCGE_OK) rc = chexel_read_back(c, c->stream, out, false);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }          // (nothing of this call is queued when it returns)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out.finish();
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// The quadrant-glyph planes of a video frame (the contract: include/ycge.h): ycge_video_blit's frame through k_video_blit_quadrants, which
// writes the sub-cell colours beside the SDR, then the fit and ycge_render_frame_quadrants' read-back.  The SDR alone: ycge_video_blit's launch
int ycge_video_blit_quadrants(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, float *out_top_bottom_sdr, float *out_quad_sdr,
                              uint16_t *out_glyphs, uint8_t *out_rgba, int32_t min_contrast)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_video_blit_quadrants";
    int rc = video_check_frame(c, fn, frame, src_w, src_h, bytes_per_pixel);
    if (rc != YCGE_OK) return rc;
    if (!out_top_bottom_sdr && !out_quad_sdr && !out_glyphs && !out_rgba)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: every destination is NULL (ask for at least one of sdr, quad_sdr, glyphs, rgba)", fn);
    rc = check_quadrant_call(c, fn, min_contrast);
    if (rc != YCGE_OK) return rc;
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const FrameOutputs::Quadrants q{out_quad_sdr, out_glyphs, out_rgba, min_contrast};
    FrameOutputs out(out_top_bottom_sdr);
    if (out_quad_sdr || out_glyphs || out_rgba) { out.quad = &q; out.quad_colours_ready = true; }
    const float *d_sdr = nullptr;
    rc = video_enqueue(c, c->stream, frame, src_w, src_h, bytes_per_pixel, c->fbW, c->fbH, c->ss, &d_sdr, out.quad ? &c->chexels.quad_sdr : nullptr);
    if (rc == YCGE_OK) rc = chexel_encode(c, c->stream, out, d_sdr, false);
    if (rc == YCGE_OK) rc = video_read_sdr(c, c->stream, d_sdr, out);
    if (rc == YCGE_OK) rc = chexel_read_back(c, c->stream, out, false);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }          // (nothing of this call is queued when it returns)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out.finish();
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the column and row tables of a video geometry as the library computes them (host only; ycge_video.cpp)
int ycge_host_video_tables(int32_t src_w, int32_t src_h, int32_t fbW, int32_t fbH, int32_t ss, int32_t *x0_out, float *wx_out, int32_t *y0_out, float *wy_out,
                           float *geometry_out)
try {
    return video_host_tables(src_w, src_h, fbW, fbH, ss, x0_out, wx_out, y0_out, wy_out, geometry_out);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: k_video_blit alone on a caller-given geometry, whatever the context's framebuffer is; returns with the SDR in the caller's array
int ycge_test_video_blit(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t fbW, int32_t fbH, int32_t ss, float *sdr_out)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return video_test_blit(c, frame, src_w, src_h, bytes_per_pixel, fbW, fbH, ss, sdr_out);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: k_video_blit_quadrants alone on a caller-given geometry (ss even), whatever the context's framebuffer is: the SDR (fbW*fbH*6) and
// the sub-cell colours (fbW*fbH*12) in the caller's arrays.  The context's quadrant planes are not touched
int ycge_test_video_blit_quadrants(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t fbW, int32_t fbH, int32_t ss,
                                   float *sdr_out, float *quad_out)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!quad_out) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_test_video_blit_quadrants: quad_out is NULL");
    return video_test_blit(c, frame, src_w, src_h, bytes_per_pixel, fbW, fbH, ss, sdr_out, quad_out);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the two threshold tables of LinearToSrgb8 (255 entries each), host only
int ycge_host_srgb_thresholds(float *f32_out, double *f64_out)
try {
    if (!f32_out || !f64_out) return YCGE_ERR_INVALID_ARG;
    const SrgbTables &t = srgb_tables();
    std::memcpy(f32_out, t.t32, 255 * sizeof(float));
    std::memcpy(f64_out, t.t64, 255 * sizeof(double));
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

// test hook: k_tonemap_quadrants alone on a caller-given hi-res buffer (fbH*2*ss rows of fbW*ss pixels) and exposure, whatever the context's
// framebuffer is.  Buffers and a tone state of its own on the context's device and stream: no frame state is touched
int ycge_test_quadrant_sdr(ycge_ctx *c, const float *hdr, int32_t fbW, int32_t fbH, int32_t ss, float exposure, float *out)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!hdr || !out || fbW <= 0 || fbH <= 0 || ss < 2 || ss > 64 || (ss & 1) || (int64_t)fbW * fbH * ss * ss > ((int64_t)1 << 26))
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_test_quadrant_sdr: bad arguments (%d x %d chexels, super_sample %d: even, 2..64)", fbW, fbH, ss);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)fbW * fbH, hi = n * 2 * ss * ss;
    DevBuf<float> in, quad; DevBuf<uint8_t> state;
    HIP_TRY(c, in.alloc(3 * hi));
    HIP_TRY(c, quad.alloc(12 * n));
    HIP_TRY(c, state.alloc(ycge_post_state_bytes()));
    uint32_t init[6] = {0, 0, 0, 0, 0, 0};
    if (ycge_post_state_bytes() != sizeof init) return c->fail(YCGE_ERR_INTERNAL, "ycge_test_quadrant_sdr: the tone state is %zu bytes, not %zu", ycge_post_state_bytes(), sizeof init);
    std::memcpy(&init[0], &exposure, 4); std::memcpy(&init[1], &exposure, 4);          // {aeExposure, effective}: as ycge_test_post_stage
    HIP_TRY(c, hipMemcpy(state.p, init, sizeof init, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(in.p, hdr, 3 * hi * sizeof(float), hipMemcpyHostToDevice));
    const int e = ycge_launch_tonemap_quadrants(in.p, fbW * ss, fbW, fbH, ss, 2.2f, 2.0f, 0.0f, state.p, quad.p, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_tonemap_quadrants launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return copy_out(c, out, quad.p, 12 * n * sizeof(float));
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: k_fit_quadrants alone on n caller-given cells of sub-cell colours, as an n x 1 framebuffer: out_rgba gets n foreground words, then
// n background words.  Either output may be NULL, not both
int ycge_test_quadrant_fit(ycge_ctx *c, const float *quad_sdr, int32_t n, int32_t min_contrast, uint16_t *out_glyphs, uint8_t *out_rgba)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!quad_sdr || n <= 0 || n > (1 << 26) || (!out_glyphs && !out_rgba) || min_contrast < 0 || min_contrast > 255)
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_test_quadrant_fit: bad arguments (n = %d, min_contrast = %d)", n, min_contrast);
    HIP_TRY(c, hipSetDevice(c->device));
    { const int rc = ensure_tables(c, c->chexels); if (rc != YCGE_OK) return rc; }
    DevBuf<float> in; DevBuf<uint16_t> glyphs; DevBuf<uint8_t> rgba;
    HIP_TRY(c, in.alloc(12 * (size_t)n));
    HIP_TRY(c, glyphs.alloc((size_t)n));
    HIP_TRY(c, rgba.alloc(8 * (size_t)n));
    HIP_TRY(c, hipMemcpy(in.p, quad_sdr, 12 * (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    const int e = ycge_launch_quadrant_fit(in.p, n, 1, c->chexels.tables.p, min_contrast, glyphs.p, rgba.p, c->compute_units, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_fit_quadrants launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = YCGE_OK;
    if (out_glyphs) rc = copy_out(c, out_glyphs, glyphs.p, 2 * (size_t)n);
    if (out_rgba && rc == YCGE_OK) rc = copy_out(c, out_rgba, rgba.p, 8 * (size_t)n);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: k_encode_chexels on caller-given SDR values (w x h chexels of {top rgb, bottom rgb}); any NULL output is skipped.  On the
// context's device and stream, with buffers of its own; returns with the bytes in the caller's arrays.
int ycge_test_encode_chexels(ycge_ctx *c, const float *sdr, int32_t w, int32_t h, uint8_t *c16, uint8_t *ansi, uint8_t *rgba)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!sdr || w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)INT32_MAX / 2 || (!c16 && !ansi && !rgba))
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_test_encode_chexels: bad arguments (w = %d, h = %d)", w, h);
    HIP_TRY(c, hipSetDevice(c->device));
    { const int rc = ensure_tables(c, c->chexels); if (rc != YCGE_OK) return rc; }
    const ChexelLayout L((size_t)w * h);
    DevBuf<float> in; DevBuf<uint8_t> out;
    HIP_TRY(c, in.alloc(6 * L.n));
    HIP_TRY(c, out.alloc(L.total));
    HIP_TRY(c, hipMemcpy(in.p, sdr, 6 * L.n * sizeof(float), hipMemcpyHostToDevice));
    const int e = ycge_launch_chexels(in.p, w, h, c->chexels.tables.p, c16 ? out.p + L.c16 : nullptr, ansi ? out.p + L.ansi : nullptr,
                                      rgba ? out.p + L.rgba : nullptr, c->compute_units, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_encode_chexels launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = YCGE_OK;
    if (c16) rc = copy_out(c, c16, out.p + L.c16, L.n);
    if (ansi && rc == YCGE_OK) rc = copy_out(c, ansi, out.p + L.ansi, 2 * L.n);
    if (rgba && rc == YCGE_OK) rc = copy_out(c, rgba, out.p + L.rgba, 8 * L.n);
    return rc;
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
