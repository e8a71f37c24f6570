// ycge_ansi.cpp - the ANSI presenter's escape streams on the device (ycge_render_frame_ansi and its kin, ycge_ansi_stream_bound; kernels:
// ycge_ansi.hip and ycge_ansi_rgb.hip over ycge_ansi_cells.hip.h).
//
// A frame of ycge_render_frame_ansi is ycge_render_frame_chexels' with the ANSI pairs alone, kept on the device: behind their encode,
// on the same stream, three launches turn them into the bytes ANSITerminalRenderer.Render() writes (ANSITerminalRenderer.cs:86-153)
// for a console over the framebuffer, and the stream's length is copied to a page-locked word.  Once the stream is synchronised, exactly
// that many bytes are copied to the caller.  The request (AnsiRequest) travels in the entry point's FrameOutputs (ycge_ctx.h) down to
// chexel_encode, chexel_read_back and ansi_enqueue: a frame whose outputs name no request issues no launch or copy of it.
//
// The delta form (ycge_render_frame_ansi_delta, ycge_video_blit_ansi_delta) keeps the pairs of the last stream it handed out in one of two
// buffers of ChexelState and writes only the cells that changed since; the contract is in include/ycge.h.  Its encode writes into the
// other buffer and a successful call flips the two: nothing is copied.  A keyframe runs the full stream's kernels on those pairs, so its
// bytes are ycge_render_frame_ansi's.
//
// The 24-bit colour forms (ycge_render_frame_ansi_rgb, ycge_render_frame_ansi_rgb_delta and the two video calls) are the same calls with
// `rgb` set in the request: the encode keeps the RGBA plane instead of the pairs, the bound counts 39 bytes a cell, and the delta compares
// against what the terminal shows under a tolerance.  One request, one launch, one delta transaction (DeltaCall) and one delivery serve
// every form; the delta state belongs to the one terminal, so a stream of either family invalidates it for both.
//
// A call is decided in three values.  Its DeltaCall compares ONE key - colour form, family, layers set or not, console, viewport, default
// colours, framebuffer - with the held one (ChexelState::delta_key) and so decides keyframe or delta.  Its AnsiPlan (plan_of) follows from
// the request and that decision: every buffer the call reads or writes with the size it must have, and where the frame's colour plane
// lies.  ensure_frame_buffers grows the buffers to the plan before anything is queued - the held plane a _delta call's encode writes
// included - and a frame in flight is queued without a join only when frame_buffers_ready finds the same plan met; chexel_encode and
// chexel_read_back take the plane's place from it (ycge_chexel.cpp, ansi_frame_plane).  launch() then fills one ycge_ansi::StreamJob
// (ycge_ansi_layers.h) - planes, geometry, defaults, full or delta, the layers and the composite's planes - and hands it to the colour
// form's one entry point, ycge_launch_ansi_indexed or ycge_launch_ansi_rgb; frames, video and the test hooks all come through it.
//
// Layers (ycge_console_set_layers): the console's other framebuffers, kept in ChexelState::layers with their colours encoded once by
// k_encode_chexels.  While any are set, launch() runs the compose pass in front of the stream kernels, which then walk the console-wide
// composite; the delta forms keep the last composite's colour and glyph planes in comp_held / glyph_held, flipped with delta_held.
//
// The quadrant-glyph forms (ycge_render_frame_ansi_quad, _quad_delta): `quad` set beside `rgb`.  The frame's plane is k_fit_quadrants' and a
// glyph plane comes with it, so EVERY such stream runs the compose pass - with no layers set, over the raytrace framebuffer alone - and walks
// the composite with the layered 24-bit kernels; its delta state is the composite's (comp_held / glyph_held), a third family beside the two.
// The video forms (ycge_video_blit_ansi_quad, _quad_delta) are video() with the same request: k_video_blit_quadrants makes the sub-cell
// colours, the encode is the fit alone, and the delta state is the family's one.
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

// The plan of r's call (AnsiPlan, ycge_ctx.h), the one place where its buffers' sizes and its frame plane's place are decided.  bound: its
// stream's; keyframe: what its DeltaCall decided; fbW x fbH: the framebuffer; layered: layers are set.  A _delta call outside the quadrant
// family holds the frame's plane for the next call; every layered or quadrant stream composes into the held pairs of console-wide planes
static AnsiPlan plan_of(const AnsiRequest &r, bool keyframe, unsigned long long bound, int fbW, int fbH, bool layered)
{
    const size_t cells = (size_t)r.cw * (size_t)r.ch, px = r.rgb ? 8 : 2;
    AnsiPlan p;
    p.rgb_palette = r.rgb;
    p.stream = bound;
    p.tile_words = 4 * (size_t)ycge_launch_ansi_tiles((uint32_t)r.cw * (uint32_t)r.ch);          // (the delta kernels keep four words a tile)
    if (r.delta && !r.quad) {
        p.held = px * (size_t)fbW * fbH;
        p.frame_in_held = keyframe || !r.rgb;          // (a 24-bit delta's write kernel fills the held plane instead)
    }
    if (layered || r.quad) {
        p.comp = px * cells; p.comp_cells = cells;
        if (r.rgb && r.delta) p.comp_cur = p.comp;
    }
    return p;
}

// every buffer of plan p and the elements it must have, handed to `each` until one answers other than YCGE_OK
template <class F>
static int each_buffer(ChexelState &X, const AnsiPlan &p, F each)
{
    int rc = each(X.ansi_stream, p.stream);
    if (rc == YCGE_OK) rc = each(X.ansi_tiles, p.tile_words);
    if (rc == YCGE_OK) rc = each(X.ansi_res, (size_t)4);
    if (rc == YCGE_OK) rc = each(X.delta_held[1 - X.delta_prev], p.held);
    for (int k = 0; k < 2 && rc == YCGE_OK; k++) {
        rc = each(X.comp_held[k], p.comp);
        if (rc == YCGE_OK) rc = each(X.glyph_held[k], p.comp_cells);
    }
    return rc == YCGE_OK ? each(X.comp_cur, p.comp_cur) : rc;
}

// whether a call of plan p finds every buffer it names as it is: one that has to grow is freed under the frames in flight that read it
static bool frame_buffers_ready(ChexelState &X, const AnsiPlan &p)
{
    if (p.rgb_palette ? !X.rgb_palette_ready : !X.ansi_palette_ready) return false;
    return each_buffer(X, p, [](auto &b, size_t n) { return b.cap < n ? YCGE_ERR_INTERNAL : YCGE_OK; }) == YCGE_OK;
}

// what a stream call makes before it queues anything: the buffers of its plan (kept while large enough), the page-locked words of what
// the scan reports, and the default colours
static int ensure_frame_buffers(ycge_ctx *c, ChexelState &X, const AnsiPlan &p, hipStream_t stream)
{
    const int rc = each_buffer(X, p, [c](auto &b, size_t n) { if (b.cap < n) HIP_TRY(c, b.alloc(n)); return (int)YCGE_OK; });
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, X.ansi_res_host.reserve(4 * sizeof(unsigned long long)));
    return p.rgb_palette ? ensure_rgb_palette(c, X, stream) : ensure_palette(c, X, stream);
}

// S's layers in the colour form rgb, composed into comp / comp_glyph
static ycge_ansi::LayersRun layers_run(const LayerStore &S, bool rgb, uint8_t *comp, uint16_t *comp_glyph)
{
    ycge_ansi::LayersRun L{};
    L.n = S.n; L.raytrace_at = S.raytrace_at; L.cells = S.cells;
    L.colours = rgb ? S.rgba.p : S.pairs.p; L.glyphs = S.glyphs.p;
    for (int k = 0; k < S.n; k++) L.rect[k] = S.rect[k];
    L.comp = comp; L.comp_glyph = comp_glyph;
    return L;
}

// r's stream as the job j describes it, and the copy of what the scan reports: a delta's {length, changed, emitted, run starts}, otherwise
// the full stream's length alone.  The caller's part of j: the planes - the framebuffer's with its size, the previous and next ones, the
// layers and the composite's - and full or delta; the rest is r's and the context's stream buffers
// flight (or NULL): the frame in flight whose stream buffer and record k_ansi_deliver fills instead of that copy
static int launch(ycge_ctx *c, ChexelState &X, hipStream_t stream, const AnsiRequest &r, ycge_ansi::StreamJob &j, const FrameOutputs *flight = nullptr)
{
    j.cw = r.cw; j.ch = r.ch; j.vx = r.vx; j.vy = r.vy; j.dfg = r.fg; j.dbg = r.bg; j.clear = r.clear; j.gap = r.gap; j.tol = r.tolerance;
    j.palette = r.rgb ? X.rgb_palette.p : reinterpret_cast<const uint8_t *>(X.ansi_palette.p + 48);
    j.tiles = X.ansi_tiles.p; j.out = X.ansi_stream.p; j.cap = X.ansi_stream.cap; j.res = X.ansi_res.p;
    int e = (r.rgb ? ycge_launch_ansi_rgb : ycge_launch_ansi_indexed)(&j, stream);
    if (e != 0)
        return c->fail(YCGE_ERR_DEVICE, "%sANSI %sstream launch failed: %s", r.quad ? "quadrant " : r.rgb ? "24-bit " : "", j.delta ? "delta " : "", hipGetErrorString((hipError_t)e));
    if (!flight) {
        HIP_TRY(c, hipMemcpyAsync(X.ansi_res_host.p, X.ansi_res.p, (j.delta ? 4 : 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        return YCGE_OK;
    }
    // a frame in flight (ycge_render_frame_async_ansi): the exact-length copy and the caller's record by k_ansi_deliver, one workgroup a CU,
    // and behind it the event the next such frame's encode waits for
    void *d_sticky = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&d_sticky, X.flight_sticky.p, 0));
    // (a length above the device stream's own size is refused as one above the caller's capacity is: no load passes the allocation)
    e = ycge_launch_ansi_deliver(j.out, j.res, flight->dev_capacity < j.cap ? flight->dev_capacity : j.cap, j.delta ? 0 : 1, flight->dev_stream, flight->dev_record, static_cast<uint32_t *>(d_sticky), c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ansi_deliver launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, X.flight_ev.ensure());
    HIP_TRY(c, hipEventRecord(X.flight_ev, stream));
    X.flight_stream = stream; X.flight_pending = true;
    return YCGE_OK;
}

int ansi_enqueue(ycge_ctx *c, hipStream_t stream, const FrameOutputs &out, const uint8_t *d_plane)
{
    ChexelState &X = c->chexels;
    const AnsiRequest &r = *out.ansi;
    { const int rc = r.rgb ? ensure_rgb_palette(c, X, stream) : ensure_palette(c, X, stream); if (rc != YCGE_OK) return rc; }
    const int held = X.delta_prev, next = 1 - X.delta_prev;
    ycge_ansi::StreamJob j{};
    j.plane = d_plane; j.fbW = c->fbW; j.fbH = c->fbH;
    j.delta = !out.keyframe;
    j.compose = X.layers.n > 0 || r.quad;
    if (!j.compose) {
        j.prev = X.delta_held[held].p; j.next = X.delta_held[next].p;
    } else {
        // (this call's composite goes where the next _delta call finds it; a 24-bit delta's write kernel fills that plane instead)
        j.frame_glyph = r.quad ? X.quad_glyphs.p : nullptr;
        j.layers = layers_run(X.layers, r.rgb, j.delta && r.rgb ? X.comp_cur.p : X.comp_held[next].p, X.glyph_held[next].p);
        j.prev = X.comp_held[held].p; j.prev_glyph = X.glyph_held[held].p; j.next = X.comp_held[next].p;
    }
    return launch(c, X, stream, r, j, out.dev_stream ? &out : nullptr);
}

} // namespace ycge_host

namespace {

// one _ansi call's transaction on the context's delta state.  A _delta call (r.delta) decides keyframe or delta, and on every way out but
// commit() makes the next call a keyframe; any other call shows the terminal its own stream next, so a later _delta call returns a keyframe
struct DeltaCall {
    ChexelState &X;
    const AnsiRequest &r;
    const bool layered;
    const ChexelState::DeltaKey key;
    bool keyframe = true, done = false;
    AnsiPlan plan;
    // bound: the stream's (check_stream_args)
    DeltaCall(ycge_ctx *c, const AnsiRequest &r_, unsigned long long bound)
        : X(c->chexels), r(r_), layered(X.layers.n > 0), key{{r_.rgb, r_.quad, layered, r_.cw, r_.ch, r_.vx, r_.vy, r_.fg, r_.bg, c->fbW, c->fbH}}
    {
        const int held = X.delta_prev;
        if (r.delta)
            keyframe = !X.delta_valid || key != X.delta_key || r.clear || r.keyframe || (!r.quad && !X.delta_held[held].p) ||
                       ((layered || r.quad) && (!X.comp_held[held].p || !X.glyph_held[held].p));
        else
            X.delta_valid = false;
        plan = plan_of(r, keyframe, bound, c->fbW, c->fbH, layered);
    }
    ~DeltaCall() { if (!done) X.delta_valid = false; }
    // what the call's frame hands out: r's stream, a keyframe or not as decided here with the plan that follows from it, and the SDR array
    FrameOutputs outputs(float *sdr) const
    {
        FrameOutputs out(sdr);
        out.ansi = &r; out.keyframe = keyframe; out.plan = plan;
        return out;
    }
    // a _delta call's stream is with the caller: this frame's pairs are `prev` from now on
    void commit()
    {
        if (!r.delta) return;
        X.delta_prev = 1 - X.delta_prev; X.delta_valid = true; X.delta_key = key;
        done = true;
    }
};

// what every entry point refuses; bound: the stream's bound in the call's colour form
int check_stream_args(ycge_ctx *c, const char *fn, const AnsiRequest &r, const uint8_t *out, size_t capacity, const size_t *out_len, unsigned long long &bound)
{
    if (!out || !out_len) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (r.cw <= 0 || r.ch <= 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: console %d x %d (both must be positive)", fn, r.cw, r.ch);
    if (r.fg < 0 || r.fg > 15 || r.bg < 0 || r.bg > 15) return c->fail(YCGE_ERR_INVALID_ARG, "%s: default colours %d, %d (ConsoleColor values 0..15)", fn, r.fg, r.bg);
    if (!stream_bound(r.cw, r.ch, r.rgb, bound) || bound > kOffsetLimit)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: the stream of a %d x %d console may reach 2^32 bytes (offsets are 32-bit)", fn, r.cw, r.ch);
    if (capacity < bound)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (%s)", fn, capacity, bound,
                       r.rgb ? "ycge_ansi_rgb_stream_bound" : "ycge_ansi_stream_bound");
    if (r.delta && (r.gap < 0 || r.gap > 8)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: merge_gap %d (0..8)", fn, r.gap);
    if (r.delta && r.rgb && (r.tolerance < 0 || r.tolerance > 255)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: tolerance %d (0..255)", fn, r.tolerance);
    return YCGE_OK;
}

// behind the stream's synchronisation: the length the device wrote, the bound check, exactly that many bytes of the device stream into
// `out` (staged when pageable; on c->stream, synchronously); then the caller's words - out_info (a _delta call's, or NULL): {keyframe,
// changed, emitted, run starts}, the counters zero for a keyframe (full: the full stream's scan wrote the length alone)
int deliver(ycge_ctx *c, ChexelState &X, const char *fn, bool full, unsigned long long bound, uint8_t *out, size_t *out_len, uint32_t *out_info)
{
    const unsigned long long *res = static_cast<const unsigned long long *>(X.ansi_res_host.p);
    const size_t len = (size_t)res[0];
    if (res[0] > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, res[0], bound);
    uint8_t *target = out;
    const bool staged = !host_memory_is_page_locked(out, len);
    if (staged) {
        HIP_TRY(c, X.stage.reserve(len));
        target = X.stage.data();
    }
    HIP_TRY(c, hipMemcpyAsync(target, X.ansi_stream.p, len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (staged) std::memcpy(out, X.stage.p, len);
    *out_len = len;
    if (out_info) {
        out_info[0] = full ? 1u : 0u;
        for (int k = 1; k < 4; k++) out_info[k] = full ? 0u : (uint32_t)res[k];
    }
    return YCGE_OK;
}

// ycge_render_frame_ansi and its three kin.  The delta forms (the contract: include/ycge.h): a keyframe is the plain call's stream, a delta
// writes the cells that changed since the last stream this context handed out; out_info is theirs alone
int frame(ycge_ctx *c, const char *fn, const AnsiRequest &r, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr,
          ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, r, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK && r.quad) rc = check_quadrant_call(c, fn, r.min_contrast);
    if (rc == YCGE_OK) rc = check_post_frame(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    DeltaCall call(c, r, bound);
    FrameOutputs out = call.outputs(out_top_bottom_sdr);
    ChexelState &X = c->chexels;
    rc = ensure_frame_buffers(c, X, call.plan, c->stream);
    if (rc != YCGE_OK) return rc;
    rc = render_frame_sync(c, &out, st);          // (its stream synchronisation: the length and the counters have arrived)
    if (rc != YCGE_OK) return rc;
    rc = deliver(c, X, fn, call.keyframe, bound, out_stream, out_len, r.delta ? out_info : nullptr);
    if (rc != YCGE_OK) return rc;
    call.commit();
    return YCGE_OK;
}

// ---- frames in flight (ycge_render_frame_async_ansi; the contract: include/ycge.h).  The call is frame() without deliver(): the stream's
// launches end in k_ansi_deliver (launch() above), which copies the exact length into the caller's page-locked buffer and fills the record,
// so nothing is waited for.  The delta state moves at queue time: DeltaCall decides keyframe or delta, commit() flips the held planes.

// what k_ansi_deliver is given: a 16-byte aligned stream buffer, page-locked over all of its capacity, and an 8-byte aligned page-locked record
int check_flight_buffers(ycge_ctx *c, const char *fn, const uint8_t *out, size_t capacity, const void *rec)
{
    if (((uintptr_t)out & 15u) != 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream %p is not 16-byte aligned", fn, (const void *)out);
    if (((uintptr_t)rec & 7u) != 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_result %p is not 8-byte aligned", fn, rec);
    if (!host_memory_is_page_locked(out, capacity))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream must be page-locked memory over all of its capacity, %zu bytes (ycge_alloc_host_buffer, or whole pages "
                                             "registered with ycge_pin_host_buffer): the device fills it while the caller runs on", fn, capacity);
    if (!host_memory_is_page_locked(rec, sizeof(ycge_ansi_async_result)))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_result must be page-locked memory (ycge_alloc_host_buffer, or whole pages registered with ycge_pin_host_buffer)", fn);
    return YCGE_OK;
}

// the sticky word of the library (join_async looks at it)
int ensure_flight(ycge_ctx *c, ChexelState &X)
{
    if (X.flight_sticky.p) return YCGE_OK;
    HIP_TRY(c, X.flight_sticky.reserve(64));
    std::memset(X.flight_sticky.p, 0, 64);
    return YCGE_OK;
}

AnsiRequest request(bool rgb, int32_t cw, int32_t ch, int32_t vx, int32_t vy, int32_t fg, int32_t bg, int32_t clear);
AnsiRequest with_delta(AnsiRequest r, int32_t merge_gap, int32_t tolerance, int32_t keyframe);

int frame_async(ycge_ctx *c, const ycge_ansi_async *q, uint8_t *out_stream, size_t capacity, ycge_ansi_async_result *out_result, float *out_top_bottom_sdr)
{
    static const char fn[] = "ycge_render_frame_async_ansi";
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!q) return c->fail(YCGE_ERR_INVALID_ARG, "%s: req must not be NULL", fn);
    if (!out_stream || !out_result) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_result must not be NULL", fn);
    AnsiRequest r = request(q->rgb != 0, q->console_w, q->console_h, q->viewport_x, q->viewport_y, q->default_fg16, q->default_bg16, q->clear_screen);
    if (!q->delta && (q->merge_gap || q->tolerance || q->keyframe))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: merge_gap %d, tolerance %d, keyframe %d on a full stream (delta = 0: all three must be 0)", fn, q->merge_gap, q->tolerance, q->keyframe);
    if (q->delta && !q->rgb && q->tolerance) return c->fail(YCGE_ERR_INVALID_ARG, "%s: tolerance %d without rgb (must be 0)", fn, q->tolerance);
    if (q->delta) r = with_delta(r, q->merge_gap, q->tolerance, q->keyframe);
    unsigned long long bound = 0;
    size_t unused = 0;
    int rc = check_stream_args(c, fn, r, out_stream, capacity, &unused, bound);
    if (rc == YCGE_OK) rc = check_flight_buffers(c, fn, out_stream, capacity, out_result);
    if (rc != YCGE_OK) return rc;
    if (out_top_bottom_sdr && !host_memory_is_page_locked(out_top_bottom_sdr, (size_t)c->fbW * c->fbH * 6 * sizeof(float)))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_top_bottom_sdr must be page-locked memory (ycge_alloc_host_buffer, or whole pages registered with ycge_pin_host_buffer)", fn);
    rc = check_in_flight(c);
    if (rc == YCGE_OK) rc = check_post_frame(c);
    if (rc != YCGE_OK) return rc;
    if (!c->taa_stream) return c->fail(YCGE_ERR_INVALID_ARG, "no second stream: frames in flight need a single-device context");
    HIP_TRY(c, hipSetDevice(c->device));
    DeltaCall call(c, r, bound);
    FrameOutputs out = call.outputs(out_top_bottom_sdr);
    ChexelState &X = c->chexels;
    if (!frame_buffers_ready(X, call.plan) || !X.flight_sticky.p) {
        // (the first call of a form or a size: the frames in flight are joined, and what the buffers' makers queued on c->stream is waited for)
        rc = join_async(c);
        if (rc == YCGE_OK) rc = ensure_frame_buffers(c, X, call.plan, c->stream);
        if (rc == YCGE_OK) rc = ensure_flight(c, X);
        if (rc != YCGE_OK) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    void *d_out = nullptr, *d_rec = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&d_out, out_stream, 0));
    HIP_TRY(c, hipHostGetDevicePointer(&d_rec, out_result, 0));
    out.dev_stream = static_cast<uint8_t *>(d_out); out.dev_record = d_rec; out.dev_capacity = capacity;
    rc = render_frame_in_flight(c, &out);
    if (rc != YCGE_OK) return rc;
    call.commit();
    return YCGE_OK;
}

// The delivery's test hook: k_ansi_deliver alone on a caller-given device stream and result words, synchronised.  groups: its workgroups
// (0: the product's grid, one a CU).  Stateless but for the context's stream buffer, which holds src afterwards
int test_deliver(ycge_ctx *c, const uint8_t *src, size_t n_src, unsigned long long length, size_t capacity, int32_t keyframe, const uint32_t *counts, int32_t groups,
                 uint8_t *out_stream, ycge_ansi_async_result *out_result)
{
    static const char fn[] = "ycge_test_ansi_deliver";
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!out_stream || !out_result || !counts || (n_src > 0 && !src) || groups < 0 || groups > 65536)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad arguments (src %p, n_src %zu, counts %p, groups %d, out_stream %p, out_result %p)", fn, (const void *)src, n_src,
                       (const void *)counts, groups, (const void *)out_stream, (const void *)out_result);
    if (length <= capacity && length > n_src) return c->fail(YCGE_ERR_INVALID_ARG, "%s: length %llu is above n_src %zu (the copy would read past the source)", fn, length, n_src);
    if (c->async_outstanding) return c->fail(YCGE_ERR_INVALID_ARG, "%s: frames are in flight on this context (ycge_wait first)", fn);
    int rc = check_flight_buffers(c, fn, out_stream, capacity, out_result);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    ChexelState &X = c->chexels;
    if (X.ansi_stream.cap < n_src || !X.ansi_stream.p) HIP_TRY(c, X.ansi_stream.alloc(n_src > 16 ? n_src : 16));
    if (!X.ansi_res.p) HIP_TRY(c, X.ansi_res.alloc(4));
    rc = ensure_flight(c, X);
    if (rc != YCGE_OK) return rc;
    if (n_src > 0) HIP_TRY(c, hipMemcpy(X.ansi_stream.p, src, n_src, hipMemcpyHostToDevice));
    const unsigned long long words[4] = {length, counts[0], counts[1], counts[2]};
    HIP_TRY(c, hipMemcpy(X.ansi_res.p, words, sizeof words, hipMemcpyHostToDevice));
    void *d_out = nullptr, *d_rec = nullptr, *d_sticky = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&d_out, out_stream, 0));
    HIP_TRY(c, hipHostGetDevicePointer(&d_rec, out_result, 0));
    HIP_TRY(c, hipHostGetDevicePointer(&d_sticky, X.flight_sticky.p, 0));
    const int e = ycge_launch_ansi_deliver(X.ansi_stream.p, X.ansi_res.p, capacity, keyframe ? 1 : 0, static_cast<uint8_t *>(d_out), d_rec, static_cast<uint32_t *>(d_sticky),
                                           groups > 0 ? groups : c->compute_units, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_ansi_deliver launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return YCGE_OK;
}

// Video mode (ycge_video.cpp): the stream of VideoRenderer.TryFlipAndBlit's chexels for the frame the host's IFrameReader shows; the
// delta forms on the same delta state: one terminal, whichever renderer the host shows on it
int video(ycge_ctx *c, const char *fn, const AnsiRequest &r, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, uint8_t *out_stream,
          size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    unsigned long long bound = 0;
    int rc = video_check_frame(c, fn, frame, src_w, src_h, bytes_per_pixel);
    if (rc == YCGE_OK) rc = check_stream_args(c, fn, r, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK && r.quad) rc = check_quadrant_call(c, fn, r.min_contrast);
    if (rc != YCGE_OK) return rc;
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    DeltaCall call(c, r, bound);
    FrameOutputs out = call.outputs(out_top_bottom_sdr);
    out.quad_colours_ready = r.quad;          // (the quadrant family: k_video_blit_quadrants writes the sub-cell colours, the encode is the fit alone)
    ChexelState &X = c->chexels;
    rc = ensure_frame_buffers(c, X, call.plan, c->stream);
    const float *d_sdr = nullptr;
    if (rc == YCGE_OK) rc = video_enqueue(c, c->stream, frame, src_w, src_h, bytes_per_pixel, c->fbW, c->fbH, c->ss, &d_sdr, r.quad ? &X.quad_sdr : nullptr);
    if (rc == YCGE_OK) rc = chexel_encode(c, c->stream, out, d_sdr, false);
    if (rc == YCGE_OK) rc = video_read_sdr(c, c->stream, d_sdr, out);
    if (rc == YCGE_OK) rc = chexel_read_back(c, c->stream, out, false);          // (the stream kernels and the copy of what they report)
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rc = deliver(c, X, fn, call.keyframe, bound, out_stream, out_len, r.delta ? out_info : nullptr);
    if (rc != YCGE_OK) return rc;
    out.finish();
    call.commit();
    return YCGE_OK;
}

// a hook's own device copy of n host elements
template <class T>
int upload(ycge_ctx *c, DevBuf<T> &b, const T *src, size_t n)
{
    HIP_TRY(c, b.alloc(n));
    HIP_TRY(c, hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return YCGE_OK;
}

// what every hook makes first: the context's buffers by the plan of r's full unlayered stream - every plane is the hook's own
int hook_begin(ycge_ctx *c, AnsiRequest r, unsigned long long bound)
{
    HIP_TRY(c, hipSetDevice(c->device));
    r.delta = r.quad = false;
    return ensure_frame_buffers(c, c->chexels, plan_of(r, true, bound, 0, 0, false), c->stream);
}

// a hook's job: launched, waited for, delivered
int hook_run(ycge_ctx *c, const char *fn, const AnsiRequest &r, ycge_ansi::StreamJob &j, unsigned long long bound, uint8_t *out_stream, size_t *out_len, uint32_t *out_info)
{
    const int rc = launch(c, c->chexels, c->stream, r, j);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return deliver(c, c->chexels, fn, !j.delta, bound, out_stream, out_len, out_info);
}

// The four test hooks: r's stream kernels alone on caller-given planes of the fbW x fbH framebuffer (`what` names cur in the refusal), with
// the geometry, defaults and refusals of the frame call; on the context's device and stream.  A delta (r.delta) runs against prev; a NULL
// prev or a clear_screen gives the keyframe.  Stateless: plane buffers of its own, the context's request and delta state untouched.
// out_shown (24-bit delta, or NULL): the next `shown` - cur after a keyframe, otherwise cur where a covered cell was emitted and prev
// elsewhere - with every fourth byte 255
int test_stream(ycge_ctx *c, const char *fn, const char *what, const AnsiRequest &r, const uint8_t *prev, const uint8_t *cur, int32_t fbW, int32_t fbH,
                uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, uint8_t *out_shown)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!cur || fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad framebuffer (%s %p, %d x %d)", fn, what, (const void *)cur, fbW, fbH);
    unsigned long long bound = 0;
    int rc = check_stream_args(c, fn, r, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK) rc = hook_begin(c, r, bound);
    if (rc != YCGE_OK) return rc;
    const bool full = !r.delta || !prev || r.clear;
    const size_t bytes = (r.rgb ? 8 : 2) * (size_t)fbW * fbH;
    DevBuf<uint8_t> in, held, next;
    rc = upload(c, in, cur, bytes);
    if (rc == YCGE_OK && !full) rc = upload(c, held, prev, bytes);
    if (rc != YCGE_OK) return rc;
    if (!full && r.rgb) {
        HIP_TRY(c, next.alloc(bytes));
        HIP_TRY(c, hipMemcpy(next.p, held.p, bytes, hipMemcpyDeviceToDevice));      // (framebuffer cells off the console keep what they held)
    }
    ycge_ansi::StreamJob j{};
    j.plane = in.p; j.fbW = fbW; j.fbH = fbH; j.delta = !full; j.prev = held.p; j.next = next.p;
    rc = hook_run(c, fn, r, j, bound, out_stream, out_len, out_info);
    if (rc != YCGE_OK || !out_shown) return rc;
    rc = copy_out(c, out_shown, full ? in.p : next.p, bytes);
    if (rc != YCGE_OK) return rc;
    for (size_t k = 3; k < bytes; k += 4) out_shown[k] = 255;
    return YCGE_OK;
}

constexpr uint64_t kLayerCellsMax = 1ull << 26;

// what ycge_console_set_layers refuses in its arguments; cells: the layers' cells in all
int check_layers(ycge_ctx *c, const char *fn, const ycge_console_layer *layers, int32_t n, int32_t raytrace_at, uint64_t &cells)
{
    if (n < 0 || n > YCGE_CONSOLE_MAX_LAYERS) return c->fail(YCGE_ERR_INVALID_ARG, "%s: n = %d (0..%d layers)", fn, n, YCGE_CONSOLE_MAX_LAYERS);
    if (raytrace_at < 0 || raytrace_at > n) return c->fail(YCGE_ERR_INVALID_ARG, "%s: raytrace_at = %d (0..n = %d)", fn, raytrace_at, n);
    if (n > 0 && !layers) return c->fail(YCGE_ERR_INVALID_ARG, "%s: layers is NULL with n = %d", fn, n);
    cells = 0;
    for (int32_t k = 0; k < n; k++) {
        if (!layers[k].cells) return c->fail(YCGE_ERR_INVALID_ARG, "%s: layers[%d].cells is NULL", fn, k);
        if (layers[k].w <= 0 || layers[k].h <= 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: layers[%d] is %d x %d (both must be positive)", fn, k, layers[k].w, layers[k].h);
        cells += (uint64_t)layers[k].w * (uint64_t)layers[k].h;
        if (cells > kLayerCellsMax) return c->fail(YCGE_ERR_INVALID_ARG, "%s: more than 2^26 cells over all layers (%llu by layers[%d])", fn, (unsigned long long)cells, k);
    }
    return YCGE_OK;
}

// checked layers into S: the cells' code units and colours uploaded, the colours encoded by k_encode_chexels as a cells x 1 framebuffer
// {top = foreground, bottom = background} into the pairs and the RGBA plane.  Synchronous on c->stream; the host's arrays are free on return
int build_layers(ycge_ctx *c, ChexelState &X, const ycge_console_layer *layers, int32_t n, int32_t raytrace_at, uint64_t cells, LayerStore &S)
{
    { const int rc = ensure_tables(c, X); if (rc != YCGE_OK) return rc; }
    std::vector<uint16_t> glyphs((size_t)cells);
    std::vector<float> sdr(6 * (size_t)cells);
    size_t at = 0;
    for (int32_t k = 0; k < n; k++) {
        const ycge_console_layer &l = layers[k];
        S.rect[k] = ycge_ansi::LayerRect{l.x, l.y, l.w, l.h, (uint32_t)at};
        const size_t count = (size_t)l.w * (size_t)l.h;
        for (size_t j = 0; j < count; j++, at++) {
            const ycge_chexel &x = l.cells[j];
            glyphs[at] = x.ch;
            for (int q = 0; q < 3; q++) { sdr[6 * at + q] = x.fg[q]; sdr[6 * at + 3 + q] = x.bg[q]; }
        }
    }
    S.n = n; S.raytrace_at = raytrace_at; S.cells = (uint32_t)cells;
    DevBuf<float> d_sdr;
    HIP_TRY(c, d_sdr.upload(sdr));
    HIP_TRY(c, S.glyphs.upload(glyphs));
    HIP_TRY(c, S.pairs.alloc(2 * (size_t)cells));
    HIP_TRY(c, S.rgba.alloc(8 * (size_t)cells));
    const int e = ycge_launch_chexels(d_sdr.p, (int)cells, 1, X.tables.p, nullptr, S.pairs.p, S.rgba.p, c->compute_units, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_encode_chexels launch failed (the layers' colours): %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return YCGE_OK;
}

// ycge_console_set_layers: all or nothing - the new store is complete before it replaces the old one
int set_layers(ycge_ctx *c, const ycge_console_layer *layers, int32_t n, int32_t raytrace_at)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    const char *fn = "ycge_console_set_layers";
    uint64_t cells = 0;
    int rc = check_layers(c, fn, layers, n, raytrace_at, cells);
    if (rc != YCGE_OK) return rc;
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    LayerStore S;
    if (n > 0) {
        rc = build_layers(c, c->chexels, layers, n, raytrace_at, cells, S);
        if (rc != YCGE_OK) return rc;
    }
    c->chexels.layers = std::move(S);
    return YCGE_OK;
}

// The layered test hook: compose and stream kernels alone on a caller-given framebuffer plane (rgb: the RGBA plane, else the pairs), layers
// and previous composite, with the geometry, defaults and refusals of the frame calls.  delta: a _delta call's rules - a NULL previous
// composite or a clear_screen gives the keyframe.  Stateless: layer store and planes of its own; the context's layers, request and delta
// state are untouched.  out_colours / out_glyphs (or NULL): the next composite - this call's, in a 24-bit delta emitted ? cur : shown
// The quadrant hooks (r.quad) come through here with frame_glyphs, the framebuffer's fbW * fbH code units, and no layers (n = 0)
int test_layers(ycge_ctx *c, const char *fn, const AnsiRequest &r, const uint8_t *plane, const uint16_t *frame_glyphs, int32_t fbW, int32_t fbH,
                const ycge_console_layer *layers, int32_t n, int32_t raytrace_at, const uint8_t *prev_colours, const uint16_t *prev_glyphs, uint8_t *out_stream,
                size_t capacity, size_t *out_len, uint32_t *out_info, uint8_t *out_colours, uint16_t *out_glyphs)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!plane || (r.quad && !frame_glyphs) || fbW <= 0 || fbH <= 0 || (int64_t)fbW * fbH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad framebuffer (plane %p, glyphs %p, %d x %d)", fn, (const void *)plane, (const void *)frame_glyphs, fbW, fbH);
    unsigned long long bound = 0;
    uint64_t cells = 0;
    int rc = check_stream_args(c, fn, r, out_stream, capacity, out_len, bound);
    if (rc == YCGE_OK) rc = check_layers(c, fn, layers, n, raytrace_at, cells);
    if (rc != YCGE_OK) return rc;
    if (n == 0 && !r.quad) return c->fail(YCGE_ERR_INVALID_ARG, "%s: n = 0 (the unlayered streams have hooks of their own)", fn);
    rc = hook_begin(c, r, bound);
    LayerStore S;
    if (rc == YCGE_OK && n > 0) rc = build_layers(c, c->chexels, layers, n, raytrace_at, cells, S);
    if (rc != YCGE_OK) return rc;
    const bool full = !r.delta || !prev_colours || !prev_glyphs || r.clear;
    const size_t console = (size_t)r.cw * (size_t)r.ch, bytes = (r.rgb ? 8 : 2) * console, fb_bytes = (r.rgb ? 8 : 2) * (size_t)fbW * fbH;
    DevBuf<uint8_t> in, comp, held, next;
    DevBuf<uint16_t> comp_glyph, held_glyph, in_glyph;
    rc = upload(c, in, plane, fb_bytes);
    if (rc == YCGE_OK && r.quad) rc = upload(c, in_glyph, frame_glyphs, (size_t)fbW * fbH);
    if (rc == YCGE_OK && !full) rc = upload(c, held, prev_colours, bytes);
    if (rc == YCGE_OK && !full) rc = upload(c, held_glyph, prev_glyphs, console);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, comp.alloc(bytes));
    HIP_TRY(c, comp_glyph.alloc(console));
    if (!full && r.rgb) HIP_TRY(c, next.alloc(bytes));
    ycge_ansi::StreamJob j{};
    j.plane = in.p; j.frame_glyph = in_glyph.p; j.fbW = fbW; j.fbH = fbH; j.delta = !full;
    j.prev = held.p; j.prev_glyph = held_glyph.p; j.next = next.p;
    j.compose = true; j.layers = layers_run(S, r.rgb, comp.p, comp_glyph.p);
    rc = hook_run(c, fn, r, j, bound, out_stream, out_len, r.delta ? out_info : nullptr);
    if (rc == YCGE_OK && out_colours) rc = copy_out(c, out_colours, !full && r.rgb ? next.p : comp.p, bytes);
    if (rc == YCGE_OK && out_glyphs) rc = copy_out(c, out_glyphs, comp_glyph.p, console * sizeof(uint16_t));
    return rc;
}

// a call's arguments as its request
AnsiRequest request(bool rgb, int32_t cw, int32_t ch, int32_t vx, int32_t vy, int32_t fg, int32_t bg, int32_t clear)
{
    AnsiRequest r;
    r.rgb = rgb; r.cw = cw; r.ch = ch; r.vx = vx; r.vy = vy; r.fg = fg; r.bg = bg; r.clear = clear != 0;
    return r;
}

AnsiRequest with_delta(AnsiRequest r, int32_t merge_gap, int32_t tolerance, int32_t keyframe)
{
    r.delta = true; r.gap = merge_gap; r.tolerance = tolerance; r.keyframe = keyframe != 0;
    return r;
}

// the quadrant-glyph family: 24-bit colour, the fit under min_contrast
AnsiRequest quad_request(int32_t cw, int32_t ch, int32_t vx, int32_t vy, int32_t fg, int32_t bg, int32_t clear, int32_t min_contrast)
{
    AnsiRequest r = request(true, cw, ch, vx, vy, fg, bg, clear);
    r.quad = true; r.min_contrast = min_contrast;
    return r;
}

int bound_call(int32_t console_w, int32_t console_h, bool rgb, size_t *bytes)
{
    unsigned long long b = 0;
    if (!bytes || console_w <= 0 || console_h <= 0 || !stream_bound(console_w, console_h, rgb, b)) return YCGE_ERR_INVALID_ARG;
    *bytes = (size_t)b;
    return YCGE_OK;
}

} // namespace

// =========================================================================== C-ABI
extern "C" {

int ycge_ansi_stream_bound(int32_t console_w, int32_t console_h, size_t *bytes)
try {
    return bound_call(console_w, console_h, false, bytes);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_ansi(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                           int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr,
                           ycge_frame_stats *st)
try {
    return frame(c, "ycge_render_frame_ansi", request(false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen), out_stream,
                 capacity, out_len, nullptr, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                         int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                         size_t *out_len, float *out_top_bottom_sdr)
try {
    return video(c, "ycge_video_blit_ansi", request(false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen), frame, src_w, src_h,
                 bytes_per_pixel, out_stream, capacity, out_len, nullptr, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_ansi_delta(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                 int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t keyframe, uint8_t *out_stream, size_t capacity,
                                 size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    const AnsiRequest r = request(false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return frame(c, "ycge_render_frame_ansi_delta", with_delta(r, merge_gap, 0, keyframe), out_stream, capacity, out_len, out_info, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_delta(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                               int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                               int32_t keyframe, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr)
try {
    const AnsiRequest r = request(false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return video(c, "ycge_video_blit_ansi_delta", with_delta(r, merge_gap, 0, keyframe), frame, src_w, src_h, bytes_per_pixel, out_stream, capacity, out_len, out_info,
                 out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

// The 24-bit colour forms (the contract: include/ycge.h): the same four calls on sRGB8 triples, the delta with a tolerance
int ycge_ansi_rgb_stream_bound(int32_t console_w, int32_t console_h, size_t *bytes)
try {
    return bound_call(console_w, console_h, true, bytes);
}
catch (...) { return ycge_host::abi_catch(nullptr); }

int ycge_render_frame_ansi_rgb(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                               int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr,
                               ycge_frame_stats *st)
try {
    return frame(c, "ycge_render_frame_ansi_rgb", request(true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen), out_stream,
                 capacity, out_len, nullptr, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_rgb(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                             int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream,
                             size_t capacity, size_t *out_len, float *out_top_bottom_sdr)
try {
    return video(c, "ycge_video_blit_ansi_rgb", request(true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen), frame, src_w,
                 src_h, bytes_per_pixel, out_stream, capacity, out_len, nullptr, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_ansi_rgb_delta(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                     int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance, int32_t keyframe, uint8_t *out_stream,
                                     size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    const AnsiRequest r = request(true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return frame(c, "ycge_render_frame_ansi_rgb_delta", with_delta(r, merge_gap, tolerance, keyframe), out_stream, capacity, out_len, out_info, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_rgb_delta(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                                   int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                                   int32_t tolerance, int32_t keyframe, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                                   float *out_top_bottom_sdr)
try {
    const AnsiRequest r = request(true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return video(c, "ycge_video_blit_ansi_rgb_delta", with_delta(r, merge_gap, tolerance, keyframe), frame, src_w, src_h, bytes_per_pixel, out_stream, capacity, out_len,
                 out_info, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

// The quadrant-glyph forms (the contract: include/ycge.h): the 24-bit calls with the fitted glyph and colours for '▀', top, bottom
int ycge_render_frame_ansi_quad(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                int32_t default_bg16, int32_t clear_screen, int32_t min_contrast, uint8_t *out_stream, size_t capacity, size_t *out_len,
                                float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    return frame(c, "ycge_render_frame_ansi_quad", quad_request(console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, min_contrast),
                 out_stream, capacity, out_len, nullptr, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_render_frame_ansi_quad_delta(ycge_ctx *c, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16,
                                      int32_t default_bg16, int32_t clear_screen, int32_t merge_gap, int32_t tolerance, int32_t keyframe, int32_t min_contrast,
                                      uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
try {
    const AnsiRequest r = quad_request(console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, min_contrast);
    return frame(c, "ycge_render_frame_ansi_quad_delta", with_delta(r, merge_gap, tolerance, keyframe), out_stream, capacity, out_len, out_info, out_top_bottom_sdr, st);
}
catch (...) { return ycge_host::abi_catch(c); }

// ... and of a video frame, on the quadrant family's delta state: one terminal, whichever renderer the host shows on it
int ycge_video_blit_ansi_quad(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                              int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t min_contrast,
                              uint8_t *out_stream, size_t capacity, size_t *out_len, float *out_top_bottom_sdr)
try {
    return video(c, "ycge_video_blit_ansi_quad", quad_request(console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, min_contrast), frame,
                 src_w, src_h, bytes_per_pixel, out_stream, capacity, out_len, nullptr, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_video_blit_ansi_quad_delta(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bytes_per_pixel, int32_t console_w, int32_t console_h,
                                    int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                                    int32_t tolerance, int32_t keyframe, int32_t min_contrast, uint8_t *out_stream, size_t capacity, size_t *out_len,
                                    uint32_t *out_info, float *out_top_bottom_sdr)
try {
    const AnsiRequest r = quad_request(console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, min_contrast);
    return video(c, "ycge_video_blit_ansi_quad_delta", with_delta(r, merge_gap, tolerance, keyframe), frame, src_w, src_h, bytes_per_pixel, out_stream, capacity,
                 out_len, out_info, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hooks: the quadrant streams' kernels alone on caller-given planes of the fbW x fbH framebuffer - glyphs, fbW * fbH code units, and
// rgba, fbW x 2 fbH RGBA8 with row 2 cy the foreground - with the geometry, defaults and refusals of the frame calls and no layers.  The
// delta: shown_colours / shown_glyphs are the console-wide composite the terminal shows (cw x 2 ch RGBA8, cw * ch code units; either NULL,
// or clear_screen: the keyframe), out_shown_colours / out_shown_glyphs (or NULL) receive the next such.  Stateless
int ycge_test_ansi_quad_stream(ycge_ctx *c, const uint16_t *glyphs, const uint8_t *rgba, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                               int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream,
                               size_t capacity, size_t *out_len)
try {
    const AnsiRequest r = quad_request(console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, 0);
    return test_layers(c, "ycge_test_ansi_quad_stream", r, rgba, glyphs, fbW, fbH, nullptr, 0, 0, nullptr, nullptr, out_stream, capacity, out_len, nullptr, nullptr, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_test_ansi_quad_delta(ycge_ctx *c, const uint8_t *shown_colours, const uint16_t *shown_glyphs, const uint16_t *glyphs, const uint8_t *rgba, int32_t fbW,
                              int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16,
                              int32_t clear_screen, int32_t merge_gap, int32_t tolerance, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                              uint8_t *out_shown_colours, uint16_t *out_shown_glyphs)
try {
    const AnsiRequest r = quad_request(console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen, 0);
    return test_layers(c, "ycge_test_ansi_quad_delta", with_delta(r, merge_gap, tolerance, 0), rgba, glyphs, fbW, fbH, nullptr, 0, 0, shown_colours, shown_glyphs,
                       out_stream, capacity, out_len, out_info, out_shown_colours, out_shown_glyphs);
}
catch (...) { return ycge_host::abi_catch(c); }

// The four frame forms with frames in flight (the contract: include/ycge.h): queued, delivered on the device, the caller's after ycge_wait
int ycge_render_frame_async_ansi(ycge_ctx *c, const ycge_ansi_async *req, uint8_t *out_stream, size_t capacity, ycge_ansi_async_result *out_result,
                                 float *out_top_bottom_sdr)
try {
    return frame_async(c, req, out_stream, capacity, out_result, out_top_bottom_sdr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: k_ansi_deliver alone on a caller-given device stream and result words (test_deliver above)
int ycge_test_ansi_deliver(ycge_ctx *c, const uint8_t *src, size_t n_src, uint64_t length, size_t capacity, int32_t keyframe, const uint32_t *counts,
                           int32_t groups, uint8_t *out_stream, ycge_ansi_async_result *out_result)
try {
    return test_deliver(c, src, n_src, length, capacity, keyframe, counts, groups, out_stream, out_result);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the stream kernels alone on caller-given ANSI pairs (fbW x fbH {fg, bg}, any values 0..255), with the geometry, defaults and
// refusals of ycge_render_frame_ansi (test_stream above)
int ycge_test_ansi_stream(ycge_ctx *c, const uint8_t *pairs, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x,
                          int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                          size_t *out_len)
try {
    const AnsiRequest r = request(false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return test_stream(c, "ycge_test_ansi_stream", "pairs", r, nullptr, pairs, fbW, fbH, out_stream, capacity, out_len, nullptr, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the delta kernels alone on caller-given pairs, prev_pairs and pairs both fbW x fbH {fg, bg}; a NULL prev_pairs or a
// clear_screen gives the keyframe (ycge_test_ansi_stream's bytes)
int ycge_test_ansi_delta(ycge_ctx *c, const uint8_t *prev_pairs, const uint8_t *pairs, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                         int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                         uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info)
try {
    const AnsiRequest r = request(false, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return test_stream(c, "ycge_test_ansi_delta", "pairs", with_delta(r, merge_gap, 0, 0), prev_pairs, pairs, fbW, fbH, out_stream, capacity, out_len, out_info, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the 24-bit stream kernels alone on a caller-given RGBA plane (fbW x 2 fbH RGBA8, row 2 cy the top half-cell, the fourth byte
// ignored), with the geometry, defaults and refusals of ycge_render_frame_ansi_rgb
int ycge_test_ansi_rgb_stream(ycge_ctx *c, const uint8_t *rgba, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h, int32_t viewport_x,
                              int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, uint8_t *out_stream, size_t capacity,
                              size_t *out_len)
try {
    const AnsiRequest r = request(true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return test_stream(c, "ycge_test_ansi_rgb_stream", "rgba", r, nullptr, rgba, fbW, fbH, out_stream, capacity, out_len, nullptr, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the 24-bit delta kernels alone on caller-given planes, shown and cur both fbW x 2 fbH RGBA8 (the fourth byte ignored); a NULL
// shown or a clear_screen gives the keyframe (ycge_test_ansi_rgb_stream's bytes).  out_shown (or NULL): the next `shown`
int ycge_test_ansi_rgb_delta(ycge_ctx *c, const uint8_t *shown, const uint8_t *cur, int32_t fbW, int32_t fbH, int32_t console_w, int32_t console_h,
                             int32_t viewport_x, int32_t viewport_y, int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t merge_gap,
                             int32_t tolerance, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info, uint8_t *out_shown)
try {
    const AnsiRequest r = request(true, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    return test_stream(c, "ycge_test_ansi_rgb_delta", "cur", with_delta(r, merge_gap, tolerance, 0), shown, cur, fbW, fbH, out_stream, capacity, out_len, out_info,
                       out_shown);
}
catch (...) { return ycge_host::abi_catch(c); }

// The console's other framebuffers (the contract: include/ycge.h): from this call on every stream call of the context writes the bytes
// Render() writes for the whole list
int ycge_console_set_layers(ycge_ctx *c, const ycge_console_layer *layers, int32_t n, int32_t raytrace_at)
try {
    return set_layers(c, layers, n, raytrace_at);
}
catch (...) { return ycge_host::abi_catch(c); }

// test hook: the compose and stream kernels alone on a caller-given framebuffer plane, layers and previous composite (test_layers above)
int ycge_test_ansi_layers(ycge_ctx *c, int32_t rgb, const uint8_t *plane, int32_t fbW, int32_t fbH, const ycge_console_layer *layers, int32_t n, int32_t raytrace_at,
                          const uint8_t *prev_colours, const uint16_t *prev_glyphs, int32_t console_w, int32_t console_h, int32_t viewport_x, int32_t viewport_y,
                          int32_t default_fg16, int32_t default_bg16, int32_t clear_screen, int32_t delta, int32_t merge_gap, int32_t tolerance, uint8_t *out_stream,
                          size_t capacity, size_t *out_len, uint32_t *out_info, uint8_t *out_colours, uint16_t *out_glyphs)
try {
    AnsiRequest r = request(rgb != 0, console_w, console_h, viewport_x, viewport_y, default_fg16, default_bg16, clear_screen);
    if (delta) r = with_delta(r, merge_gap, rgb ? tolerance : 0, 0);
    return test_layers(c, "ycge_test_ansi_layers", r, plane, nullptr, fbW, fbH, layers, n, raytrace_at, prev_colours, prev_glyphs, out_stream, capacity, out_len, out_info, out_colours, out_glyphs);
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
