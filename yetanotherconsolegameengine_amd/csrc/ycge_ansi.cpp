// ycge_ansi.cpp - the ANSI presenter's escape stream on the device (ycge_render_frame_ansi, ycge_ansi_stream_bound; kernels:
// ycge_ansi.hip).
//
// A frame of ycge_render_frame_ansi is ycge_render_frame_chexels' with the ANSI pairs alone, kept on the device: behind their encode,
// on the same stream, three launches turn them into the bytes ANSITerminalRenderer.Render() writes (ANSITerminalRenderer.cs:86-153)
// for a console over the framebuffer, and the stream's length is copied to a page-locked word.  Once the stream is synchronised, exactly
// that many bytes are copied to the caller.  The request lives in ChexelState for the length of one call (a scope guard clears it; on an
// error return also every latched destination), so no other entry point issues a launch or copy of it.
//
// The delta form (ycge_render_frame_ansi_delta, ycge_video_blit_ansi_delta; kernels: ycge_ansi_delta.hip) keeps the pairs of the last
// stream it handed out in one of two buffers of ChexelState and writes only the cells that changed since; the contract is in
// include/ycge.h.  Its encode writes into the other buffer and a successful call flips the two: nothing is copied.  A keyframe runs the
// full stream's kernels on those pairs, so its bytes are ycge_render_frame_ansi's.
//
// The 24-bit colour forms (ycge_render_frame_ansi_rgb, ycge_render_frame_ansi_rgb_delta and the two video calls; kernels:
// ycge_ansi_rgb.hip) are the same calls with `rgb` set: the encode keeps the RGBA plane instead of the pairs, the bound counts 39 bytes a
// cell, and the delta compares against what the terminal shows (ChexelState::delta_shown) under a tolerance.  One request guard, one delta
// state machine and one delivery serve both families; the state belongs to the one terminal, so a stream of either family invalidates it
// for both.
//
// The default cell's colours are ansi(palette16[k]): k_encode_chexels run once on the 16 palette colours, so no second formula exists.
#include "ycge_ctx.h"

namespace {

// Chexel.cs:11-29, the palette entries that ChexelColor(ConsoleColor) holds as color_f32 (the same table as ycge_chexel.hip's)
const float kPalette16[16][3] = {
    {0.00f, 0.00f, 0.00f}, {0.00f, 0.00f, 0.50f}, {0.00f, 0.50f, 0.00f}, {0.00f, 0.50f, 0.50f},
    {0.50f, 0.00f, 0.00f}, {0.50f, 0.00f, 0.50f}, {0.50f, 0.50f, 0.00f}, {0.75f, 0.75f, 0.75f},
    {0.50f, 0.50f, 0.50f}, {0.00f, 0.00f, 1.00f}, {0.00f, 1.00f, 0.00f}, {0.00f, 1.00f, 1.00f},
    {1.00f, 0.00f, 0.00f}, {1.00f, 0.00f, 1.00f}, {1.00f, 1.00f, 0.00f}, {1.00f, 1.00f, 1.00f}};

constexpr unsigned long long kOffsetLimit = 0xffffffffull;       // the kernels' offsets are 32-bit

// the stream's upper bound: ESC[2J ESC[H, ESC[0m, each row's ESC[<y+1>;1H, and 23 bytes a cell (the longest escape, 20, and '▀', 3);
// false when it does not fit a size_t.  rgb: 39 bytes a cell (the longest 24-bit escape, 36)
bool stream_bound(int32_t cw, int32_t ch, bool rgb, unsigned long long &bytes)
{
    unsigned __int128 b = 7 + 4 + (unsigned __int128)(rgb ? 39 : 23) * (uint64_t)cw * (uint64_t)ch + (unsigned __int128)5 * (uint64_t)ch;
    for (int64_t lo = 1, d = 1; lo <= ch; lo *= 10, d++)           // the rows numbered lo .. min(ch, 10 lo - 1) have d digits
        b += (unsigned __int128)d * (uint64_t)((lo * 10 - 1 < ch ? lo * 10 - 1 : ch) - lo + 1);
    if (b > (unsigned __int128)SIZE_MAX) return false;
    bytes = (unsigned long long)b;
    return true;
}

} // namespace

namespace ycge_host {

// the 16 default indices, on `stream`: k_encode_chexels on the palette as 8 chexels {palette[2 k], palette[2 k + 1]}
static int ensure_palette(ycge_ctx *c, ChexelState &X, hipStream_t stream)
{
    if (X.ansi_palette_ready) return YCGE_OK;
    { const int rc = ensure_tables(c, X); if (rc != YCGE_OK) return rc; }
    if (!X.ansi_palette.p) HIP_TRY(c, X.ansi_palette.alloc(48 + 4));
    HIP_TRY(c, hipMemcpy(X.ansi_palette.p, kPalette16, sizeof kPalette16, hipMemcpyHostToDevice));
    const int e = ycge_launch_chexels(X.ansi_palette.p, 8, 1, X.tables.p, nullptr, reinterpret_cast<uint8_t *>(X.ansi_palette.p + 48), nullptr,
                                      c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_encode_chexels launch failed (the default colours): %s", hipGetErrorString((hipError_t)e));
    X.ansi_palette_ready = true;
    return YCGE_OK;
}

// ... and their sRGB8 triples: the same encoder on the same 8 chexels, its RGBA plane (8 x 2 words)
static int ensure_rgb_palette(ycge_ctx *c, ChexelState &X, hipStream_t stream)
{
    if (X.rgb_palette_ready) return YCGE_OK;
    { const int rc = ensure_palette(c, X, stream); if (rc != YCGE_OK) return rc; }
    if (!X.rgb_palette.p) HIP_TRY(c, X.rgb_palette.alloc(16 * 4));
    const int e = ycge_launch_chexels(X.ansi_palette.p, 8, 1, X.tables.p, nullptr, nullptr, X.rgb_palette.p, c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_encode_chexels launch failed (the default colours' triples): %s", hipGetErrorString((hipError_t)e));
    X.rgb_palette_ready = true;
    return YCGE_OK;
}

// the buffers of a cw x ch stream whose bound is `bound` (kept while large enough) and the default colours (rgb: their triples too)
static int ensure_ansi(ycge_ctx *c, ChexelState &X, int32_t cw, int32_t ch, unsigned long long bound, hipStream_t stream, bool rgb = false)
{
    if (X.ansi_stream.cap < bound) HIP_TRY(c, X.ansi_stream.alloc(bound));
    const uint32_t tiles = ycge_launch_ansi_tiles((uint32_t)cw * (uint32_t)ch);
    if (X.ansi_tiles.cap < 4 * (size_t)tiles) HIP_TRY(c, X.ansi_tiles.alloc(4 * (size_t)tiles));          // (the delta kernels keep four words a tile)
    if (!X.ansi_len.p) HIP_TRY(c, X.ansi_len.alloc(1));
    HIP_TRY(c, X.ansi_len_host.reserve(sizeof(unsigned long long)));
    return rgb ? ensure_rgb_palette(c, X, stream) : ensure_palette(c, X, stream);
}

static int launch_stream(ycge_ctx *c, ChexelState &X, hipStream_t stream, const uint8_t *d_pairs, int fbW, int fbH)
{
    const int e = ycge_launch_ansi_stream(d_pairs, fbW, fbH, X.ansi_cw, X.ansi_ch, X.ansi_vx, X.ansi_vy, reinterpret_cast<const uint8_t *>(X.ansi_palette.p + 48),
                                          X.ansi_fg, X.ansi_bg, X.ansi_clear, X.ansi_tiles.p, X.ansi_stream.p, X.ansi_stream.cap, X.ansi_len.p, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "ANSI stream launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(X.ansi_len_host.p, X.ansi_len.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

// the delta stream of d_pairs against d_prev for the request in X, and the copy of {length, changed, emitted, run starts}
static int launch_delta(ycge_ctx *c, ChexelState &X, hipStream_t stream, const uint8_t *d_pairs, const uint8_t *d_prev, int fbW, int fbH)
{
    if (!X.delta_res.p) HIP_TRY(c, X.delta_res.alloc(4));
    HIP_TRY(c, X.delta_res_host.reserve(4 * sizeof(unsigned long long)));
    const int e = ycge_launch_ansi_delta(d_pairs, d_prev, fbW, fbH, X.ansi_cw, X.ansi_ch, X.ansi_vx, X.ansi_vy, reinterpret_cast<const uint8_t *>(X.ansi_palette.p + 48),
                                         X.ansi_fg, X.ansi_bg, X.delta_gap, X.ansi_tiles.p, X.ansi_stream.p, X.ansi_stream.cap, X.delta_res.p, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "ANSI delta stream launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(X.delta_res_host.p, X.delta_res.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

// the 24-bit forms of the two: d_rgba the frame's RGBA plane; d_shown what the terminal displays, d_next the plane that receives the next `shown`
static int launch_rgb_stream(ycge_ctx *c, ChexelState &X, hipStream_t stream, const uint8_t *d_rgba, int fbW, int fbH)
{
    const int e = ycge_launch_ansi_rgb_stream(d_rgba, fbW, fbH, X.ansi_cw, X.ansi_ch, X.ansi_vx, X.ansi_vy, X.rgb_palette.p, X.ansi_fg, X.ansi_bg, X.ansi_clear,
                                              X.ansi_tiles.p, X.ansi_stream.p, X.ansi_stream.cap, X.ansi_len.p, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "24-bit ANSI stream launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(X.ansi_len_host.p, X.ansi_len.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

static int launch_rgb_delta(ycge_ctx *c, ChexelState &X, hipStream_t stream, const uint8_t *d_rgba, const uint8_t *d_shown, uint8_t *d_next, int fbW, int fbH)
{
    if (!X.delta_res.p) HIP_TRY(c, X.delta_res.alloc(4));
    HIP_TRY(c, X.delta_res_host.reserve(4 * sizeof(unsigned long long)));
    const int e = ycge_launch_ansi_rgb_delta(d_rgba, d_shown, d_next, fbW, fbH, X.ansi_cw, X.ansi_ch, X.ansi_vx, X.ansi_vy, X.rgb_palette.p, X.ansi_fg, X.ansi_bg,
                                             X.delta_gap, X.delta_tol, X.ansi_tiles.p, X.ansi_stream.p, X.ansi_stream.cap, X.delta_res.p, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "24-bit ANSI delta stream launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(X.delta_res_host.p, X.delta_res.p, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

int ansi_enqueue(ycge_ctx *c, hipStream_t stream, const uint8_t *d_pairs)
{
    ChexelState &X = c->chexels;
    if (X.ansi_rgb) {                                                 // (d_pairs: the RGBA plane)
        { const int rc = ensure_rgb_palette(c, X, stream); if (rc != YCGE_OK) return rc; }
        if (X.delta_on && !X.delta_full)
            return launch_rgb_delta(c, X, stream, d_pairs, X.delta_shown[X.delta_prev].p, X.delta_shown[1 - X.delta_prev].p, c->fbW, c->fbH);
        return launch_rgb_stream(c, X, stream, d_pairs, c->fbW, c->fbH);
    }
    { const int rc = ensure_palette(c, X, stream); if (rc != YCGE_OK) return rc; }
    if (X.delta_on && !X.delta_full) return launch_delta(c, X, stream, d_pairs, X.delta_pairs[X.delta_prev].p, c->fbW, c->fbH);
    return launch_stream(c, X, stream, d_pairs, c->fbW, c->fbH);
}

} // namespace ycge_host

namespace {

// one _ansi call: sets the request, and clears it on every way out (the SDR staging: render_frame_sync's own guard)
struct AnsiCall {
    ycge_ctx *c;
    AnsiCall(ycge_ctx *c_, bool rgb, int32_t cw, int32_t ch, int32_t vx, int32_t vy, int32_t fg, int32_t bg, int32_t clear) : c(c_)
    {
        ChexelState &X = c->chexels;
        X.on = true; X.dst[0] = X.dst[1] = X.dst[2] = nullptr;
        X.drop_staged();
        X.ansi_on = true; X.ansi_rgb = rgb;
        X.ansi_cw = cw; X.ansi_ch = ch; X.ansi_vx = vx; X.ansi_vy = vy; X.ansi_fg = fg; X.ansi_bg = bg; X.ansi_clear = clear != 0;
    }
    ~AnsiCall()
    {
        ChexelState &X = c->chexels;
        X.on = false; X.ansi_on = false; X.ansi_rgb = false;
        X.drop_staged();
    }
};

// what every entry point refuses; bound: the stream's bound in the call's colour form
int check_stream_args(ycge_ctx *c, const char *fn, bool rgb, int32_t cw, int32_t ch, int32_t fg, int32_t bg, const uint8_t *out, size_t capacity,
                      const size_t *out_len, unsigned long long &bound)
{
    if (!out || !out_len) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (cw <= 0 || ch <= 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: console %d x %d (both must be positive)", fn, cw, ch);
    if (fg < 0 || fg > 15 || bg < 0 || bg > 15) return c->fail(YCGE_ERR_INVALID_ARG, "%s: default colours %d, %d (ConsoleColor values 0..15)", fn, fg, bg);
    if (!stream_bound(cw, ch, rgb, bound) || bound > kOffsetLimit)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: the stream of a %d x %d console may reach 2^32 bytes (offsets are 32-bit)", fn, cw, ch);
    if (capacity < bound)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (%s)", fn, capacity, bound,
                       rgb ? "ycge_ansi_rgb_stream_bound" : "ycge_ansi_stream_bound");
    return YCGE_OK;
}

// exactly len bytes of the device stream into `out` (staged when pageable), on c->stream, synchronously
int copy_stream(ycge_ctx *c, ChexelState &X, uint8_t *out, size_t len)
{
    uint8_t *target = out;
    const bool staged = !host_memory_is_page_locked(out, len);
    if (staged) {
        HIP_TRY(c, X.stage.reserve(len));
        target = X.stage.data();
    }
    HIP_TRY(c, hipMemcpyAsync(target, X.ansi_stream.p, len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (staged) std::memcpy(out, X.stage.p, len);
    return YCGE_OK;
}

// one _delta call behind an AnsiCall: decides keyframe or delta, and on every way out but commit() makes the next call a keyframe
struct DeltaCall {
    ycge_ctx *c;
    int32_t key[8];
    bool done = false;
    bool rgb;
    DeltaCall(ycge_ctx *c_, bool rgb_, int32_t cw, int32_t ch, int32_t vx, int32_t vy, int32_t fg, int32_t bg, int32_t clear, int32_t gap, int32_t tol,
              int32_t keyframe)
        : c(c_), key{cw, ch, vx, vy, fg, bg, c_->fbW, c_->fbH}, rgb(rgb_)
    {
        ChexelState &X = c->chexels;
        X.delta_on = true; X.delta_gap = gap; X.delta_tol = tol;
        const DevBuf<uint8_t> &held = rgb ? X.delta_shown[X.delta_prev] : X.delta_pairs[X.delta_prev];
        X.delta_full = !X.delta_valid || X.delta_rgb != rgb || !held.p || std::memcmp(key, X.delta_key, sizeof key) != 0 || clear != 0 || keyframe != 0;
    }
    ~DeltaCall()
    {
        ChexelState &X = c->chexels;
        X.delta_on = false;
        if (!done) X.delta_valid = false;
    }
    // the stream is with the caller: this frame's pairs are `prev` from now on
    void commit()
    {
        ChexelState &X = c->chexels;
        X.delta_prev = 1 - X.delta_prev; X.delta_valid = true; X.delta_rgb = rgb;
        std::memcpy(X.delta_key, key, sizeof key);
        done = true;
    }
};

int check_merge_gap(ycge_ctx *c, const char *fn, int32_t gap)
{
    if (gap < 0 || gap > 8) return c->fail(YCGE_ERR_INVALID_ARG, "%s: merge_gap %d (0..8)", fn, gap);
    return YCGE_OK;
}

int check_tolerance(ycge_ctx *c, const char *fn, int32_t tol)
{
    if (tol < 0 || tol > 255) return c->fail(YCGE_ERR_INVALID_ARG, "%s: tolerance %d (0..255)", fn, tol);
    return YCGE_OK;
}

// behind the stream's synchronisation: the length and the counters the device wrote (full: a keyframe, whose length the full stream's scan
// wrote), the bound check, the stream's copy; then the caller's words
int deliver_delta(ycge_ctx *c, ChexelState &X, const char *fn, bool full, unsigned long long bound, uint8_t *out_stream, size_t *out_len, uint32_t *out_info)
{
    const unsigned long long *res = static_cast<const unsigned long long *>(full ? X.ansi_len_host.p : X.delta_res_host.p);
    const unsigned long long len = res[0];
    if (len > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, len, bound);
    const int rc = copy_stream(c, X, out_stream, (size_t)len);
    if (rc != YCGE_OK) return rc;
    *out_len = (size_t)len;
    if (out_info) {
        out_info[0] = full ? 1u : 0u;
        for (int k = 1; k < 4; k++) out_info[k] = full ? 0u : (uint32_t)res[k];
    }
    return YCGE_OK;
}

// ycge_render_frame_ansi (rgb: ycge_render_frame_ansi_rgb)
int frame_ansi(ycge_ctx *c, const char *fn, bool rgb, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
               int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr, ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, rgb, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    // (the exchange of the one-process RCCL form packs lean slabs when slab_albedo = 0: no albedo reaches the denoise stage)
    if (c->exchange_mode == YCGE_EXCHANGE_RCCL && !c->cfg.slab_albedo)
        return c->fail(YCGE_ERR_INVALID_ARG, "lean slabs (config.slab_albedo = 0) carry no albedo: the denoise stage cannot run");
    HIP_TRY(c, hipSetDevice(c->device));
    AnsiCall call(c, rgb, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    ChexelState &X = c->chexels;
    X.delta_valid = false;                                            // (the terminal shows this stream next: a later _delta call returns a keyframe)
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream, rgb);
    if (rc != YCGE_OK) return rc;
    rc = render_frame_sync(c, out_top_bottom_sdr, true, st);          // (its stream synchronisation: the length has arrived)
    if (rc != YCGE_OK) return rc;
    const unsigned long long len = *static_cast<const unsigned long long *>(X.ansi_len_host.p);
    if (len > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, len, bound);
    rc = copy_stream(c, X, out_stream, (size_t)len);
    if (rc != YCGE_OK) return rc;
    *out_len = (size_t)len;
    return YCGE_OK;
}

// Video mode (ycge_video.cpp): the stream of VideoRenderer.TryFlipAndBlit's chexels for the frame the host's IFrameReader shows
int video_ansi(ycge_ctx *c, const char *fn, bool rgb, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w,
               int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream,
               size_t capacity, size_t *out_len, float *out_top_bottom_sdr)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    unsigned long long bound = 0;
    int rc = video_check_frame(c, fn, frame, src_w, src_h, bytes_per_pixel);
    if (rc == YCGE_OK) rc = check_stream_args(c, fn, rgb, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    AnsiCall call(c, rgb, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    StagedSdrGuard staged(c);
    ChexelState &X = c->chexels;
    X.delta_valid = false;                                            // (as in ycge_render_frame_ansi)
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream, rgb);
    const float *d_sdr = nullptr;
    if (rc == YCGE_OK) rc = video_enqueue(c, c->stream, frame, src_w, src_h, bytes_per_pixel, c->fbW, c->fbH, c->ss, &d_sdr);
    if (rc == YCGE_OK) rc = chexel_encode(c, c->stream, d_sdr, false);
    if (rc == YCGE_OK) rc = video_read_sdr(c, c->stream, d_sdr, out_top_bottom_sdr);
    if (rc == YCGE_OK) rc = chexel_read_back(c, c->stream, false);          // (the stream kernels and the length's copy)
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long len = *static_cast<const unsigned long long *>(X.ansi_len_host.p);
    if (len > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, len, bound);
    rc = copy_stream(c, X, out_stream, (size_t)len);
    if (rc != YCGE_OK) return rc;
    finish_staged_sdr(c);
    *out_len = (size_t)len;
    return YCGE_OK;
}

// The delta form of ycge_render_frame_ansi (the contract: include/ycge.h): a keyframe is that call's stream, a delta writes the cells that
// changed since the last stream this context handed out
// (rgb: ycge_render_frame_ansi_rgb_delta, which alone reads `tolerance`)
int frame_ansi_delta(ycge_ctx *c, const char *fn, bool rgb, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                     int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance, int32_t keyframe, uint8_t *out_stream, size_t capacity,
                     size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, rgb, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK) rc = check_merge_gap(c, fn, merge_gap);
    if (rc == YCGE_OK && rgb) rc = check_tolerance(c, fn, tolerance);
    if (rc != YCGE_OK) return rc;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (c->exchange_mode == YCGE_EXCHANGE_RCCL && !c->cfg.slab_albedo)
        return c->fail(YCGE_ERR_INVALID_ARG, "lean slabs (config.slab_albedo = 0) carry no albedo: the denoise stage cannot run");
    HIP_TRY(c, hipSetDevice(c->device));
    AnsiCall call(c, rgb, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    DeltaCall delta(c, rgb, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, merge_gap, tolerance, keyframe);
    ChexelState &X = c->chexels;
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream, rgb);
    if (rc != YCGE_OK) return rc;
    rc = render_frame_sync(c, out_top_bottom_sdr, true, st);          // (its stream synchronisation: the length and the counters have arrived)
    if (rc != YCGE_OK) return rc;
    rc = deliver_delta(c, X, fn, X.delta_full, bound, out_stream, out_len, out_info);
    if (rc != YCGE_OK) return rc;
    delta.commit();
    return YCGE_OK;
}

// ... and of ycge_video_blit_ansi, on the same delta state: one terminal, whichever renderer the host shows on it
int video_ansi_delta(ycge_ctx *c, const char *fn, bool rgb, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w,
                     int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                     int32_t tolerance, int32_t keyframe, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    unsigned long long bound = 0;
    int rc = video_check_frame(c, fn, frame, src_w, src_h, bytes_per_pixel);
    if (rc == YCGE_OK) rc = check_stream_args(c, fn, rgb, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK) rc = check_merge_gap(c, fn, merge_gap);
    if (rc == YCGE_OK && rgb) rc = check_tolerance(c, fn, tolerance);
    if (rc != YCGE_OK) return rc;
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    AnsiCall call(c, rgb, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    DeltaCall delta(c, rgb, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, merge_gap, tolerance, keyframe);
    StagedSdrGuard staged(c);
    ChexelState &X = c->chexels;
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream, rgb);
    const float *d_sdr = nullptr;
    if (rc == YCGE_OK) rc = video_enqueue(c, c->stream, frame, src_w, src_h, bytes_per_pixel, c->fbW, c->fbH, c->ss, &d_sdr);
    if (rc == YCGE_OK) rc = chexel_encode(c, c->stream, d_sdr, false);
    if (rc == YCGE_OK) rc = video_read_sdr(c, c->stream, d_sdr, out_top_bottom_sdr);
    if (rc == YCGE_OK) rc = chexel_read_back(c, c->stream, false);          // (the stream kernels and the copy of what they report)
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = deliver_delta(c, X, fn, X.delta_full, bound, out_stream, out_len, out_info);
    if (rc != YCGE_OK) return rc;
    finish_staged_sdr(c);
    delta.commit();
    return YCGE_OK;
}

} // namespace

// =========================================================================== C-ABI
extern "C" {

int ycge_ansi_stream_bound(int32_t console_w, int32_t console_h, size_t *bytes)
try {
    unsigned long long b = 0;
    if (!bytes || console_w <= 0 || console_h <= 0 || !stream_bound(console_w, console_h, false, b)) return YCGE_ERR_INVALID_ARG;
    *bytes = (size_t)b;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_ansi(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                           int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr,
                           ycge_frame_stats *st)
try {
    return frame_ansi(c, "ycge_render_frame_ansi", false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, out_stream, capacity,
                      out_len, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                         int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                         size_t *out_len, float *out_top_bottom_sdr)
try {
    return video_ansi(c, "ycge_video_blit_ansi", false, frame, src_w, src_h, bytes_per_pixel, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16,
                      clear_screen, out_stream, capacity, out_len, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_ansi_delta(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                 int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t keyframe, uint8_t *out_stream, size_t capacity,
                                 size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    return frame_ansi_delta(c, "ycge_render_frame_ansi_delta", false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, merge_gap,
                            0, keyframe, out_stream, capacity, out_len, out_info, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_delta(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                               int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                               int32_t keyframe, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr)
try {
    return video_ansi_delta(c, "ycge_video_blit_ansi_delta", false, frame, src_w, src_h, bytes_per_pixel, console_w, console_h, viewport_x, viewport_y, default_fg16,
                            default_bg16, clear_screen, merge_gap, 0, keyframe, out_stream, capacity, out_len, out_info, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

// The 24-bit colour forms (the contract: include/ycge.h): the same four calls on sRGB8 triples, the delta with a tolerance
int ycge_ansi_rgb_stream_bound(int32_t console_w, int32_t console_h, size_t *bytes)
try {
    unsigned long long b = 0;
    if (!bytes || console_w <= 0 || console_h <= 0 || !stream_bound(console_w, console_h, true, b)) return YCGE_ERR_INVALID_ARG;
    *bytes = (size_t)b;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_ansi_rgb(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                               int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr,
                               ycge_frame_stats *st)
try {
    return frame_ansi(c, "ycge_render_frame_ansi_rgb", true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, out_stream,
                      capacity, out_len, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_rgb(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                             int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream,
                             size_t capacity, size_t *out_len, float *out_top_bottom_sdr)
try {
    return video_ansi(c, "ycge_video_blit_ansi_rgb", true, frame, src_w, src_h, bytes_per_pixel, console_w, console_h, viewport_x, viewport_y, default_fg16,
                      default_bg16, clear_screen, out_stream, capacity, out_len, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_ansi_rgb_delta(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                     int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance, int32_t keyframe, uint8_t *out_stream,
                                     size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    return frame_ansi_delta(c, "ycge_render_frame_ansi_rgb_delta", true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen,
                            merge_gap, tolerance, keyframe, out_stream, capacity, out_len, out_info, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_rgb_delta(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                                   int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                                   int32_t tolerance, int32_t keyframe, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                                   float *out_top_bottom_sdr)
try {
    return video_ansi_delta(c, "ycge_video_blit_ansi_rgb_delta", true, frame, src_w, src_h, bytes_per_pixel, console_w, console_h, viewport_x, viewport_y,
                            default_fg16, default_bg16, clear_screen, merge_gap, tolerance, keyframe, out_stream, capacity, out_len, out_info, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the stream kernels alone on caller-given ANSI pairs (fbW x fbH {fg, bg}, any values 0..255), with the geometry, defaults and
// refusals of ycge_render_frame_ansi; on the context's device and stream, with a pairs buffer of its own
int ycge_test_ansi_stream(ycge_ctx *c, const uint8_t *pairs, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x,
                          int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                          size_t *out_len)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_test_ansi_stream";
    if (!pairs || fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad framebuffer (pairs %p, %d x %d)", fn, (const void *)pairs, fbW, fbH);
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, false, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ChexelState &X = c->chexels;
    X.ansi_cw = console_w; X.ansi_ch = console_h; X.ansi_vx = viewport_x; X.ansi_vy = viewport_y;
    X.ansi_fg = default_fg16; X.ansi_bg = default_bg16; X.ansi_clear = clear_screen != 0;
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream);
    if (rc != YCGE_OK) return rc;
    DevBuf<uint8_t> in;
    HIP_TRY(c, in.alloc(2 * (size_t)fbW * fbH));
    HIP_TRY(c, hipMemcpy(in.p, pairs, 2 * (size_t)fbW * fbH, hipMemcpyHostToDevice));
    rc = launch_stream(c, X, c->stream, in.p, fbW, fbH);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long len = *static_cast<const unsigned long long *>(X.ansi_len_host.p);
    if (len > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, len, bound);
    rc = copy_stream(c, X, out_stream, (size_t)len);
    if (rc != YCGE_OK) return rc;
    *out_len = (size_t)len;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the delta kernels alone on caller-given pairs, prev_pairs and pairs both fbW x fbH {fg, bg}; a NULL prev_pairs or a
// clear_screen gives the keyframe (ycge_test_ansi_stream's bytes).  Stateless: pair buffers of its own, the context's delta state untouched.
int ycge_test_ansi_delta(ycge_ctx *c, const uint8_t *prev_pairs, const uint8_t *pairs, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                         int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                         uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_test_ansi_delta";
    if (!pairs || fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad framebuffer (pairs %p, %d x %d)", fn, (const void *)pairs, fbW, fbH);
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, false, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK) rc = check_merge_gap(c, fn, merge_gap);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ChexelState &X = c->chexels;
    X.ansi_cw = console_w; X.ansi_ch = console_h; X.ansi_vx = viewport_x; X.ansi_vy = viewport_y;
    X.ansi_fg = default_fg16; X.ansi_bg = default_bg16; X.ansi_clear = clear_screen != 0;
    X.delta_gap = merge_gap;
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream);
    if (rc != YCGE_OK) return rc;
    const bool full = !prev_pairs || clear_screen != 0;
    const size_t bytes = 2 * (size_t)fbW * fbH;
    DevBuf<uint8_t> in, prev;
    HIP_TRY(c, in.alloc(bytes));
    HIP_TRY(c, hipMemcpy(in.p, pairs, bytes, hipMemcpyHostToDevice));
    if (!full) {
        HIP_TRY(c, prev.alloc(bytes));
        HIP_TRY(c, hipMemcpy(prev.p, prev_pairs, bytes, hipMemcpyHostToDevice));
    }
    rc = full ? launch_stream(c, X, c->stream, in.p, fbW, fbH) : launch_delta(c, X, c->stream, in.p, prev.p, fbW, fbH);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return deliver_delta(c, X, fn, full, bound, out_stream, out_len, out_info);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the 24-bit stream kernels alone on a caller-given RGBA plane (fbW x 2 fbH RGBA8, row 2 cy the top half-cell, the fourth byte
// ignored), with the geometry, defaults and refusals of ycge_render_frame_ansi_rgb; a plane buffer of its own
int ycge_test_ansi_rgb_stream(ycge_ctx *c, const uint8_t *rgba, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x,
                              int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                              size_t *out_len)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_test_ansi_rgb_stream";
    if (!rgba || fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad framebuffer (rgba %p, %d x %d)", fn, (const void *)rgba, fbW, fbH);
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, true, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ChexelState &X = c->chexels;
    X.ansi_cw = console_w; X.ansi_ch = console_h; X.ansi_vx = viewport_x; X.ansi_vy = viewport_y;
    X.ansi_fg = default_fg16; X.ansi_bg = default_bg16; X.ansi_clear = clear_screen != 0;
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream, true);
    if (rc != YCGE_OK) return rc;
    const size_t bytes = 8 * (size_t)fbW * fbH;
    DevBuf<uint8_t> in;
    HIP_TRY(c, in.alloc(bytes));
    HIP_TRY(c, hipMemcpy(in.p, rgba, bytes, hipMemcpyHostToDevice));
    rc = launch_rgb_stream(c, X, c->stream, in.p, fbW, fbH);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return deliver_delta(c, X, fn, true, bound, out_stream, out_len, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the 24-bit delta kernels alone on caller-given planes, shown and cur both fbW x 2 fbH RGBA8 (the fourth byte ignored); a NULL
// shown or a clear_screen gives the keyframe (ycge_test_ansi_rgb_stream's bytes).  out_shown (or NULL): the next `shown` - cur after a
// keyframe, otherwise cur where a covered cell was emitted and shown elsewhere - with every fourth byte 255.  Stateless: planes of its own,
// the context's delta state untouched.
int ycge_test_ansi_rgb_delta(ycge_ctx *c, const uint8_t *shown, const uint8_t *cur, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                             int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                             int32_t tolerance, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, uint8_t *out_shown)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_test_ansi_rgb_delta";
    if (!cur || fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad framebuffer (cur %p, %d x %d)", fn, (const void *)cur, fbW, fbH);
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, true, console_w, console_h, default_fg16, default_bg16, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK) rc = check_merge_gap(c, fn, merge_gap);
    if (rc == YCGE_OK) rc = check_tolerance(c, fn, tolerance);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ChexelState &X = c->chexels;
    X.ansi_cw = console_w; X.ansi_ch = console_h; X.ansi_vx = viewport_x; X.ansi_vy = viewport_y;
    X.ansi_fg = default_fg16; X.ansi_bg = default_bg16; X.ansi_clear = clear_screen != 0;
    X.delta_gap = merge_gap; X.delta_tol = tolerance;
    rc = ensure_ansi(c, X, console_w, console_h, bound, c->stream, true);
    if (rc != YCGE_OK) return rc;
    const bool full = !shown || clear_screen != 0;
    const size_t bytes = 8 * (size_t)fbW * fbH;
    DevBuf<uint8_t> in, prev, next;
    HIP_TRY(c, in.alloc(bytes));
    HIP_TRY(c, hipMemcpy(in.p, cur, bytes, hipMemcpyHostToDevice));
    if (!full) {
        HIP_TRY(c, prev.alloc(bytes));
        HIP_TRY(c, next.alloc(bytes));
        HIP_TRY(c, hipMemcpy(prev.p, shown, bytes, hipMemcpyHostToDevice));
        HIP_TRY(c, hipMemcpy(next.p, prev.p, bytes, hipMemcpyDeviceToDevice));      // (framebuffer cells off the console keep what they held)
    }
    rc = full ? launch_rgb_stream(c, X, c->stream, in.p, fbW, fbH) : launch_rgb_delta(c, X, c->stream, in.p, prev.p, next.p, fbW, fbH);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = deliver_delta(c, X, fn, full, bound, out_stream, out_len, out_info);
    if (rc != YCGE_OK || !out_shown) return rc;
    rc = copy_out(c, out_shown, full ? in.p : next.p, bytes);
    if (rc != YCGE_OK) return rc;
    for (size_t k = 3; k < bytes; k += 4) out_shown[k] = 255;
    return YCGE_OK;
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
