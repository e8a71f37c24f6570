// ycge_sixel.cpp - the sixel presenter (ycge_render_frame_pixels, ycge_render_frame_sixel, ycge_sixel_stream_bound, their delta and Video
// mode forms; kernels: ycge_sixel.hip, k_video_pixels of ycge_video.hip; the contract: include/ycge.h).
//
// A frame of these calls is ycge_render_frame's with the post stage, plus k_sixel_pixels behind the tonemap on the same stream - every
// hi-res sample of the denoised buffer mapped, encoded to sRGB8 and quantised to a register of the 6 x 6 x 6 cube - and for a stream the
// encoder's launches on that register plane, then the copies of what the caller asked for.  What the caller asked for is the entry point's
// FrameOutputs::Pixels: chexel_encode and chexel_read_back hand a frame that names it to sixel_encode and sixel_read_back below, and a frame
// that names none issues no launch or copy of it.  The stream's parts 1 to 5 depend on the geometry and the arguments alone: the host
// builds them (stream_header) and the context keeps them on the device until another geometry or viewport asks for others.
//
// ycge_sixel_encode_host and ycge_sixel_encode_delta_host are the same streams in plain C++ from register planes (ycge_sixel_host.cpp, free of
// HIP and of this context): the yardsticks of the kernels on a machine without a device, and under YCGE_SIXEL_HOST=1 the encoders of the
// stream calls and of the stream hooks, on the planes read back.
//
// A Video mode call (ycge_video_blit_pixels / _sixel / _sixel_delta) is ycge_video_blit's upload, k_video_pixels on the uploaded frame -
// every hi-res sample of the blit, encoded and quantised - beside k_video_blit where the SDR is asked for, and the same encoder.
// The _sixel_delta calls hold the register plane of the last stream handed out (SixelState::held) as one more family of the context's
// delta state (ChexelState::delta_valid / delta_key): SixelDeltaCall below is the transaction, as DeltaCall of ycge_ansi.cpp is the ANSI families'.
#include "ycge_ctx.h"
#include "ycge_sixel_host.h"

#include <cstdlib>
#include <string>
#include <vector>

namespace {

constexpr int32_t kMaxRows = 6 * 65535;                              // a band is a row of k_sixel_presence's grid

using ycge_sixel_host::stream_bound;
using ycge_sixel_host::stream_header;

bool host_encoder_asked()
{
    const char *e = std::getenv("YCGE_SIXEL_HOST");
    return e && e[0] && !(e[0] == '0' && !e[1]);
}

// the encoder's buffers for a W x H plane, and the header on the device: grown before anything is queued
int ensure_encoder(ycge_ctx *c, SixelState &S, int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, unsigned long long bound, bool delta = false)
{
    const size_t bands = (size_t)(H + 5) / 6, max_lines = bands * (size_t)(6 * (int64_t)W < 216 ? 6 * W : 216);
    if (S.last1.cap < bands * 216) HIP_TRY(c, S.last1.alloc(bands * 216));
    if (S.lines.cap < max_lines) HIP_TRY(c, S.lines.alloc(max_lines));
    if (S.line_bytes.cap < max_lines) HIP_TRY(c, S.line_bytes.alloc(max_lines));
    if (!S.meta.p) HIP_TRY(c, S.meta.alloc(4));
    if (!S.res.p) HIP_TRY(c, S.res.alloc(4));
    if (S.stream.cap < bound) HIP_TRY(c, S.stream.alloc((size_t)bound));
    HIP_TRY(c, S.res_host.reserve(64));
    if (delta && S.span.cap < 2 * bands) HIP_TRY(c, S.span.alloc(2 * bands));
    const std::array<int32_t, 5> key{{W, H, vx, vy, delta ? 2 : (clear ? 1 : 0)}};
    if (key != S.header_key || !S.header.p) {
        const std::string h = stream_header(W, H, vx, vy, clear, delta);
        if (S.header.cap < h.size()) HIP_TRY(c, S.header.alloc(h.size()));
        S.header_key = {{0, 0, 0, 0, 0}};
        HIP_TRY(c, hipMemcpy(S.header.p, h.data(), h.size(), hipMemcpyHostToDevice));
        S.header_key = key; S.header_bytes = (uint32_t)h.size();
    }
    return YCGE_OK;
}

// d_prev: the delta against that plane (k_sixel_diff in front, the DELTA instances), the length and the three counts copied
int launch_encoder(ycge_ctx *c, SixelState &S, const uint8_t *d_index, int32_t W, int32_t H, unsigned long long bound, hipStream_t stream, const uint8_t *d_prev = nullptr)
{
    const size_t bands = (size_t)(H + 5) / 6, max_lines = bands * (size_t)(6 * (int64_t)W < 216 ? 6 * W : 216);
    const int e = ycge_launch_sixel_encode(d_index, W, H, S.last1.p, S.lines.p, S.line_bytes.p, (uint32_t)max_lines, S.meta.p, S.header.p, S.header_bytes, S.stream.p,
                                           (uint32_t)bound, S.res.p, c->compute_units, stream, d_prev, d_prev ? S.span.p : nullptr);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "the sixel encoder's launches failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(S.res_host.p, S.res.p, (d_prev ? 4 : 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

// ---- the adaptive palette (kernels: ycge_sixel_palette.hip; the block's layout: ycge_sixel_host.h)
using namespace ycge_sixel_host;          // (kPal*, KeptPalette, palette_*)
constexpr int64_t kPaletteMaxPixels = kPalettePixels;

// the histogram, the block and the words its head is copied to: made before anything is queued
int ensure_palette(ycge_ctx *c, SixelState &S)
{
    if (!S.pal_hist.p) HIP_TRY(c, S.pal_hist.alloc((size_t)4 * kPaletteBins));
    if (!S.pal_block.p) { S.pal_kept = false; HIP_TRY(c, S.pal_block.alloc(kPalBlockBytes)); }
    HIP_TRY(c, S.res_host.reserve(kPalHeadBytes));
    return YCGE_OK;
}

// the PAL encoder's buffers for a W x H plane (256 registers a band), and the stream's parts 1 to 4 on the device
int ensure_encoder_palette(ycge_ctx *c, SixelState &S, int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, unsigned long long bound)
{
    const size_t bands = (size_t)(H + 5) / 6, max_lines = bands * (size_t)(6 * (int64_t)W < 256 ? 6 * W : 256);
    if (S.last1.cap < bands * 256) HIP_TRY(c, S.last1.alloc(bands * 256));
    if (S.lines.cap < max_lines) HIP_TRY(c, S.lines.alloc(max_lines));
    if (S.line_bytes.cap < max_lines) HIP_TRY(c, S.line_bytes.alloc(max_lines));
    if (!S.meta.p) HIP_TRY(c, S.meta.alloc(4));
    if (S.stream.cap < bound) HIP_TRY(c, S.stream.alloc((size_t)bound));
    const std::array<int32_t, 5> key{{W, H, vx, vy, clear ? 1 : 0}};
    if (key != S.pal_prefix_key || !S.pal_prefix.p) {
        const std::string h = stream_prefix(W, H, vx, vy, clear);
        if (S.pal_prefix.cap < h.size()) HIP_TRY(c, S.pal_prefix.alloc(h.size()));
        S.pal_prefix_key = {{0, 0, 0, 0, 0}};
        HIP_TRY(c, hipMemcpy(S.pal_prefix.p, h.data(), h.size(), hipMemcpyHostToDevice));
        S.pal_prefix_key = key; S.pal_prefix_bytes = (uint32_t)h.size();
    }
    return YCGE_OK;
}

// the copy of the block's head - {length, n, ..., bytes, percentages} - into res_host: one small copy a call
int copy_palette_head(ycge_ctx *c, SixelState &S, hipStream_t stream)
{
    HIP_TRY(c, hipMemcpyAsync(S.res_host.p, S.pal_block.p, kPalHeadBytes, hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

// the PAL encoder on the register plane k_pal_remap wrote: the definitions and their length come from the block, the length goes into it
int launch_encoder_palette(ycge_ctx *c, SixelState &S, const uint8_t *d_index, int32_t W, int32_t H, unsigned long long bound, hipStream_t stream)
{
    const size_t bands = (size_t)(H + 5) / 6, max_lines = bands * (size_t)(6 * (int64_t)W < 256 ? 6 * W : 256);
    const int e = ycge_launch_sixel_encode_palette(d_index, W, H, S.last1.p, S.lines.p, S.line_bytes.p, (uint32_t)max_lines, S.meta.p, S.pal_prefix.p, S.pal_prefix_bytes,
                                                   S.pal_block.p + kPalDefs, reinterpret_cast<const uint32_t *>(S.pal_block.p + kPalDefsBytes), S.stream.p,
                                                   (uint32_t)bound, reinterpret_cast<unsigned long long *>(S.pal_block.p + kPalLength), c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "the sixel encoder's launches failed: %s", hipGetErrorString((hipError_t)e));
    return copy_palette_head(c, S, stream);
}

// the palette stage on the RGBA plane at d_rgba: built (build) or kept, the registers into d_index (NULL: none)
int launch_palette(ycge_ctx *c, SixelState &S, const uint8_t *d_rgba, int32_t W, int32_t H, bool build, uint8_t *d_index, hipStream_t stream)
{
    const int e = ycge_launch_sixel_palette(d_rgba, W, H, build ? 1 : 0, S.pal_hist.p, S.pal_block.p, d_index, c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "the palette stage's launches failed: %s", hipGetErrorString((hipError_t)e));
    return YCGE_OK;
}

// the head as it arrived in res_host -> the caller's palette and count
void palette_out(const SixelState &S, uint8_t *out_palette, int32_t *out_count, uint8_t *out_pct = nullptr)
{
    const uint8_t *head = static_cast<const uint8_t *>(S.res_host.p);
    if (out_palette) std::memcpy(out_palette, head + kPalRgba, 1024);
    if (out_pct) std::memcpy(out_pct, head + kPalPct, 768);
    if (out_count) { uint32_t n; std::memcpy(&n, head + kPalCount, 4); *out_count = (int32_t)n; }
}

// YCGE_SIXEL_HOST: the palette stage and the encoder in plain C++ on the RGBA plane read back (rgba; index: n bytes of scratch).  build: the
// palette of this picture, which goes to the device block as the kept one; else the kept block's, fetched.  Synchronous
int palette_stream_on_host(ycge_ctx *c, SixelState &S, const char *fn, const uint8_t *rgba, uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear,
                           bool build, uint8_t *out_stream, size_t capacity, size_t *out_len, uint8_t *out_palette, int32_t *out_count)
{
    std::vector<KeptPalette> keep(1);
    KeptPalette &K = keep[0];
    std::vector<uint8_t> block(kPalBlockBytes, 0);
    if (build) {
        palette_build(rgba, (size_t)W * H, K);
        const std::string defs = palette_definitions(K.pct, K.count);
        const uint32_t n = (uint32_t)K.count, bytes = (uint32_t)defs.size();
        std::memcpy(&block[kPalCount], &n, 4); std::memcpy(&block[kPalDefsBytes], &bytes, 4);
        std::memcpy(&block[kPalRgba], K.rgba, 1024); std::memcpy(&block[kPalPct], K.pct, 768);
        std::memcpy(&block[kPalDefs], defs.data(), defs.size()); std::memcpy(&block[kPalTable], K.table, kPaletteBins);
        HIP_TRY(c, hipMemcpy(S.pal_block.p, block.data(), block.size(), hipMemcpyHostToDevice));
    } else {
        HIP_TRY(c, hipMemcpy(block.data(), S.pal_block.p, block.size(), hipMemcpyDeviceToHost));
        uint32_t n; std::memcpy(&n, &block[kPalCount], 4);
        K.count = (int32_t)n;
        std::memcpy(K.rgba, &block[kPalRgba], 1024); std::memcpy(K.pct, &block[kPalPct], 768); std::memcpy(K.table, &block[kPalTable], kPaletteBins);
    }
    palette_map(rgba, (size_t)W * H, K, index);
    const int rc = encode_palette(index, K.pct, K.count, W, H, vx, vy, clear, out_stream, capacity, out_len);
    if (rc != YCGE_OK) return c->fail(rc, "%s: the host encoder refused the frame's register plane", fn);
    if (out_palette) std::memcpy(out_palette, K.rgba, 1024);
    if (out_count) *out_count = K.count;
    return YCGE_OK;
}

// what every _palette call refuses beside its frame's own refusals; bound: the stream's (a stream call)
int check_palette_call(ycge_ctx *c, const char *fn, bool stream, int64_t W, int64_t H, int32_t vx, int32_t vy, int32_t hold, const uint8_t *out_stream, size_t capacity,
                       const size_t *out_len, unsigned long long &bound)
{
    if (stream && (!out_stream || !out_len)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (stream && (vx < 0 || vy < 0)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: viewport (%d, %d) (neither may be negative)", fn, vx, vy);
    if (hold < 0 || hold > 1) return c->fail(YCGE_ERR_INVALID_ARG, "%s: hold %d (0 or 1)", fn, hold);
    if (W * H > kPaletteMaxPixels)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: a picture of %lld x %lld pixels (the adaptive palette takes at most 2^24: a bin's byte sums are 32-bit)", fn, (long long)W, (long long)H);
    if (!stream) return YCGE_OK;
    if (!palette_stream_bound(W, H, bound) || H > kMaxRows)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: the stream of %lld x %lld pixels may reach 2^32 bytes (offsets are 32-bit), or has more than %d rows", fn, (long long)W, (long long)H, kMaxRows);
    if (capacity < bound) return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (ycge_sixel_palette_stream_bound)", fn, capacity, bound);
    return YCGE_OK;
}

// behind the stream's synchronisation: the length the device wrote, the bound check, exactly that many bytes into `out` (staged when pageable)
// info (a delta): {0, changed bands, pixels painted, lines} as k_sixel_scan counted them
int deliver(ycge_ctx *c, SixelState &S, const char *fn, unsigned long long bound, uint8_t *out, size_t *out_len, uint32_t *info = nullptr)
{
    const unsigned long long *res = static_cast<const unsigned long long *>(S.res_host.p);
    const unsigned long long len = res[0];
    if (info) { info[0] = 0; info[1] = (uint32_t)res[1]; info[2] = (uint32_t)res[2]; info[3] = (uint32_t)res[3]; }
    if (len > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, len, bound);
    uint8_t *target = out;
    const bool staged = !host_memory_is_page_locked(out, (size_t)len);
    if (staged) {
        HIP_TRY(c, S.stage.reserve((size_t)len));
        target = S.stage.data();
    }
    HIP_TRY(c, hipMemcpyAsync(target, S.stream.p, (size_t)len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (staged) std::memcpy(out, S.stage.p, (size_t)len);
    *out_len = (size_t)len;
    return YCGE_OK;
}

// what both frame calls refuse, before any device work
int check_pixel_frame(ycge_ctx *c, const char *fn, int32_t dither)
{
    if (dither < 0 || dither > 1) return c->fail(YCGE_ERR_INVALID_ARG, "%s: dither %d (0 or 1)", fn, dither);
    const int rc = check_post_frame(c);
    if (rc != YCGE_OK) return rc;
    if (c->hiW != c->fbW * c->ss || c->hiH != 2 * c->fbH * c->ss || (int64_t)c->hiW * c->hiH > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: a picture of %d x %d pixels (the hi-res buffer of a %d x %d framebuffer at super_sample %d; at most 2^30 pixels)", fn,
                       c->hiW, c->hiH, c->fbW, c->fbH, c->ss);
    return YCGE_OK;
}

// the planes of the frame at hand and the thresholds, made before the frame is queued
int ensure_planes(ycge_ctx *c, SixelState &S, bool rgba)
{
    const size_t n = (size_t)c->hiW * c->hiH;
    if (rgba && S.rgba.cap < 4 * n) HIP_TRY(c, S.rgba.alloc(4 * n));
    if (S.index.cap < n) HIP_TRY(c, S.index.alloc(n));
    return ensure_tables(c, c->chexels);
}

} // namespace

namespace ycge_host {

int sixel_encode(ycge_ctx *c, hipStream_t stream, const FrameOutputs &asked)
{
    SixelState &S = c->sixel;
    const FrameOutputs::Pixels &q = *asked.pixels;
    const int W = c->hiW, H = c->hiH;
    uint8_t *plane = q.dev_index ? q.dev_index : S.index.p;
    if (!plane || (!q.dev_index && S.index.cap < (size_t)W * H) || (q.rgba && S.rgba.cap < 4 * (size_t)W * H) || !c->chexels.tables.p)
        return c->fail(YCGE_ERR_INTERNAL, "sixel_encode: the planes of a %d x %d picture are not on the device", W, H);
    if (q.pal) {
        // the RGBA plane alone from k_sixel_pixels, then the palette stage on it (YCGE_SIXEL_HOST and a stream: the host's, on the plane read back)
        if (S.rgba.cap < 4 * (size_t)W * H || !S.pal_block.p || !S.pal_hist.p) return c->fail(YCGE_ERR_INTERNAL, "sixel_encode: the palette's buffers are not on the device");
        const int e = ycge_launch_sixel_pixels(c->denoised, W, H, 2.2f, 2.0f, 0.0f, c->tone_state.p, c->chexels.tables.p, 0, S.rgba.p, nullptr, c->compute_units, stream);
        if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_sixel_pixels launch failed: %s", hipGetErrorString((hipError_t)e));
        if (q.stream && host_encoder_asked()) return YCGE_OK;
        return launch_palette(c, S, S.rgba.p, W, H, q.pal == 2, (q.stream || q.index) ? plane : nullptr, stream);
    }
    // k_sixel_pixels on the buffer and exposure state the tonemap in front of this read
    const int e = ycge_launch_sixel_pixels(c->denoised, W, H, 2.2f, 2.0f, 0.0f, c->tone_state.p, c->chexels.tables.p, q.dither, q.rgba ? S.rgba.p : nullptr, plane,
                                           c->compute_units, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_sixel_pixels launch failed: %s", hipGetErrorString((hipError_t)e));
    return YCGE_OK;
}

// the planes' copies - pageable destinations staged one behind the other - and for a stream the encoder's launches and the length's copy
// (YCGE_SIXEL_HOST: the register plane's copy into the staging instead, for the host encoder)
static int planes_read_back(ycge_ctx *c, hipStream_t stream, FrameOutputs &out, int32_t W, int32_t H)
{
    SixelState &S = c->sixel;
    const FrameOutputs::Pixels &q = *out.pixels;
    const size_t n = (size_t)W * H;
    const bool host_plane = q.stream && host_encoder_asked();
    const uint8_t *plane = q.dev_index ? q.dev_index : S.index.p;
    void *dst[2] = {q.rgba, q.index};
    const void *src[2] = {S.rgba.p, plane};
    const size_t bytes[2] = {4 * n, n}, off[2] = {0, 4 * n};
    size_t staged = host_plane ? 5 * n + n + (q.dev_prev ? n : 0) : 0;          // (the host encoder's plane, and a delta's prev: behind both)
    if (host_plane && q.pal) staged = 5 * n + 4 * n + n;                        // (the adaptive palette on the host: the RGBA plane, and room for its registers)
    for (int k = 0; k < 2; k++)
        if (dst[k] && !host_memory_is_page_locked(dst[k], bytes[k]) && staged < off[k] + bytes[k]) staged = off[k] + bytes[k];
    HIP_TRY(c, S.stage.reserve(staged));
    for (int k = 0; k < 2; k++) {
        if (!dst[k]) continue;
        void *target = dst[k];
        if (!host_memory_is_page_locked(dst[k], bytes[k])) target = out.redirect(dst[k], S.stage.data() + off[k], bytes[k]);
        HIP_TRY(c, hipMemcpyAsync(target, src[k], bytes[k], hipMemcpyDeviceToHost, stream));
    }
    if (q.pal) {
        if (host_plane) { HIP_TRY(c, hipMemcpyAsync(S.stage.data() + 5 * n, S.rgba.p, 4 * n, hipMemcpyDeviceToHost, stream)); return YCGE_OK; }
        if (!q.stream) return copy_palette_head(c, S, stream);
        unsigned long long pal_bound = 0;
        if (!palette_stream_bound(W, H, pal_bound)) return c->fail(YCGE_ERR_INTERNAL, "sixel_read_back: no bound for %d x %d pixels", W, H);
        return launch_encoder_palette(c, S, plane, W, H, pal_bound, stream);
    }
    if (!q.stream) return YCGE_OK;
    if (host_plane) {
        HIP_TRY(c, hipMemcpyAsync(S.stage.data() + 5 * n, plane, n, hipMemcpyDeviceToHost, stream));
        if (q.dev_prev) HIP_TRY(c, hipMemcpyAsync(S.stage.data() + 6 * n, q.dev_prev, n, hipMemcpyDeviceToHost, stream));
        return YCGE_OK;
    }
    unsigned long long bound = 0;
    if (!stream_bound(W, H, bound)) return c->fail(YCGE_ERR_INTERNAL, "sixel_read_back: no bound for %d x %d pixels", W, H);
    return launch_encoder(c, S, plane, W, H, bound, stream, q.dev_prev);
}

int sixel_read_back(ycge_ctx *c, hipStream_t stream, FrameOutputs &out) { return planes_read_back(c, stream, out, c->hiW, c->hiH); }

// ---- the bodies of the exports and hooks (the C-ABI with its exception barrier: ycge_chexel.cpp)

int sixel_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes)
{
    unsigned long long b = 0;
    if (!bytes || !stream_bound(px_w, px_h, b)) return YCGE_ERR_INVALID_ARG;
    *bytes = (size_t)b;
    return YCGE_OK;
}

int sixel_encode_host(const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len)
{
    return ycge_sixel_host::encode(index, W, H, vx, vy, clear, out, capacity, out_len);
}

int sixel_encode_delta_host(const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity, size_t *out_len,
                            uint32_t *out_info)
{
    return ycge_sixel_host::encode_delta(prev, index, W, H, vx, vy, out, capacity, out_len, out_info);
}

int sixel_frame_pixels(ycge_ctx *c, float *out_top_bottom_sdr, uint8_t *out_rgba, uint8_t *out_index, int32_t dither, ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_render_frame_pixels";
    if (!out_top_bottom_sdr && !out_rgba && !out_index)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: every destination is NULL (ask for at least one of sdr, rgba, index)", fn);
    int rc = check_pixel_frame(c, fn, dither);
    if (rc != YCGE_OK) return rc;
    const FrameOutputs::Pixels q{out_rgba, out_index, dither, false, 0, 0, false};
    FrameOutputs out(out_top_bottom_sdr);
    if (out_rgba || out_index) {          // (the SDR alone: ycge_render_frame's frame)
        out.pixels = &q;
        rc = join_async(c);
        if (rc != YCGE_OK) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        rc = ensure_planes(c, c->sixel, out_rgba != nullptr);
        if (rc != YCGE_OK) return rc;
    }
    return render_frame_sync(c, &out, st);
}

int sixel_frame_stream(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t dither, uint8_t *out_stream, size_t capacity,
                            size_t *out_len, float *out_top_bottom_sdr, ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_render_frame_sixel";
    if (!out_stream || !out_len) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (viewport_x < 0 || viewport_y < 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: viewport (%d, %d) (neither may be negative)", fn, viewport_x, viewport_y);
    int rc = check_pixel_frame(c, fn, dither);
    if (rc != YCGE_OK) return rc;
    unsigned long long bound = 0;
    if (!stream_bound(c->hiW, c->hiH, bound) || c->hiH > kMaxRows)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: the stream of %d x %d pixels may reach 2^32 bytes (offsets are 32-bit), or has more than %d rows", fn, c->hiW, c->hiH, kMaxRows);
    if (capacity < bound) return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (ycge_sixel_stream_bound)", fn, capacity, bound);
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    SixelState &S = c->sixel;
    rc = ensure_planes(c, S, false);
    const bool host_plane = host_encoder_asked();
    if (rc == YCGE_OK && !host_plane) rc = ensure_encoder(c, S, c->hiW, c->hiH, viewport_x, viewport_y, clear_screen != 0, bound);
    if (rc != YCGE_OK) return rc;
    const FrameOutputs::Pixels q{nullptr, nullptr, dither, true, viewport_x, viewport_y, clear_screen != 0};
    FrameOutputs out(out_top_bottom_sdr);
    out.pixels = &q;
    rc = render_frame_sync(c, &out, st);          // (its stream synchronisation: the length has arrived)
    if (rc != YCGE_OK) return rc;
    if (host_plane) {
        const size_t n = (size_t)c->hiW * c->hiH;
        rc = sixel_encode_host(S.stage.data() + 5 * n, c->hiW, c->hiH, viewport_x, viewport_y, clear_screen, out_stream, capacity, out_len);
        if (rc != YCGE_OK) return c->fail(rc, "%s: the host encoder refused the frame's register plane", fn);
    } else {
        rc = deliver(c, S, fn, bound, out_stream, out_len);
        if (rc != YCGE_OK) return rc;
    }
    c->chexels.delta_valid = false;          // (the picture lies over the terminal's cells: the next _delta call of any family is a keyframe)
    return YCGE_OK;
}

// test hook: the pixel stage alone on a caller's hi-res buffer (2 fbH ss rows of fbW ss samples) under `exposure`, whatever the context's
// framebuffer is.  Buffers and a tone state of its own on the context's device and stream: no frame state is touched.  Either output may be NULL
int sixel_test_pixels(ycge_ctx *c, const float *hdr, int32_t fbW, int32_t fbH, int32_t ss, float exposure, int32_t dither, uint8_t *out_rgba, uint8_t *out_index)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!hdr || (!out_rgba && !out_index) || fbW <= 0 || fbH <= 0 || ss < 1 || ss > 64 || (int64_t)fbW * fbH * ss * ss > ((int64_t)1 << 26) || dither < 0 || dither > 1)
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_test_pixels: bad arguments (%d x %d chexels, super_sample %d: 1..64, dither %d: 0 or 1)", fbW, fbH, ss, dither);
    HIP_TRY(c, hipSetDevice(c->device));
    { const int rc = ensure_tables(c, c->chexels); if (rc != YCGE_OK) return rc; }
    const int W = fbW * ss, H = 2 * fbH * ss;
    const size_t n = (size_t)W * H;
    DevBuf<float> in; DevBuf<uint8_t> state, rgba, index;
    HIP_TRY(c, in.alloc(3 * n));
    HIP_TRY(c, rgba.alloc(4 * n));
    HIP_TRY(c, index.alloc(n));
    HIP_TRY(c, state.alloc(ycge_post_state_bytes()));
    uint32_t init[6] = {0, 0, 0, 0, 0, 0};
    if (ycge_post_state_bytes() != sizeof init) return c->fail(YCGE_ERR_INTERNAL, "ycge_test_pixels: the tone state is %zu bytes, not %zu", ycge_post_state_bytes(), sizeof init);
    std::memcpy(&init[0], &exposure, 4); std::memcpy(&init[1], &exposure, 4);          // {aeExposure, effective}: as ycge_test_post_stage
    HIP_TRY(c, hipMemcpy(state.p, init, sizeof init, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(in.p, hdr, 3 * n * sizeof(float), hipMemcpyHostToDevice));
    const int e = ycge_launch_sixel_pixels(in.p, W, H, 2.2f, 2.0f, 0.0f, state.p, c->chexels.tables.p, dither, out_rgba ? rgba.p : nullptr, out_index ? index.p : nullptr,
                                           c->compute_units, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_sixel_pixels launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = YCGE_OK;
    if (out_rgba) rc = copy_out(c, out_rgba, rgba.p, 4 * n);
    if (out_index && rc == YCGE_OK) rc = copy_out(c, out_index, index.p, n);
    return rc;
}

// test hook: the encoder's kernels alone on a caller's register plane of any W x H whose bound fits (values of 216 or more are refused here,
// on the host), with buffers of its own: nothing of the context's sixel or delta state is touched.  YCGE_SIXEL_HOST: the host encoder
int sixel_test_stream(ycge_ctx *c, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_test_sixel_stream";
    unsigned long long bound = 0;
    if (!index || !out || !out_len || vx < 0 || vy < 0 || !stream_bound(W, H, bound) || H > kMaxRows)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad arguments (%d x %d pixels at (%d, %d))", fn, W, H, vx, vy);
    if (capacity < bound) return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (ycge_sixel_stream_bound)", fn, capacity, bound);
    const size_t n = (size_t)W * H;
    for (size_t i = 0; i < n; i++)
        if (index[i] >= 216) return c->fail(YCGE_ERR_INVALID_ARG, "%s: register %d at pixel %zu (0..215)", fn, (int)index[i], i);
    if (host_encoder_asked()) return sixel_encode_host(index, W, H, vx, vy, clear, out, capacity, out_len);
    HIP_TRY(c, hipSetDevice(c->device));
    SixelState S;
    DevBuf<uint8_t> plane;
    HIP_TRY(c, plane.alloc(n));
    { const int rc = ensure_encoder(c, S, W, H, vx, vy, clear != 0, bound); if (rc != YCGE_OK) return rc; }
    HIP_TRY(c, hipMemcpy(plane.p, index, n, hipMemcpyHostToDevice));
    { const int rc = launch_encoder(c, S, plane.p, W, H, bound, c->stream); if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; } }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return deliver(c, S, fn, bound, out, out_len);
}

} // namespace ycge_host

namespace {

// One _sixel_delta call's transaction on the context's delta state, frames and video alike: keyframe or delta is decided here, the call's
// registers go to held[next], and every way out but commit() leaves the next _delta call of any family a keyframe
struct SixelDeltaCall {
    ChexelState &X;
    SixelState &S;
    const ChexelState::DeltaKey key;
    bool keyframe = true;
    int next = 0;
    SixelDeltaCall(ycge_ctx *c, int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool asked)
        : X(c->chexels), S(c->sixel), key{{SixelState::kSixelFamily, 0, 0, W, H, vx, vy, 0, 0, c->fbW, c->fbH}}
    {
        const DevBuf<uint8_t> &prev = S.held[S.held_prev];
        keyframe = !X.delta_valid || key != X.delta_key || clear || asked || !prev.p || prev.cap < (size_t)W * H;
        next = 1 - S.held_prev;
        X.delta_valid = false;
    }
    const uint8_t *prev() const { return keyframe ? nullptr : S.held[S.held_prev].p; }
    // the stream is with the caller: this call's plane is `prev` from now on
    void commit() { S.held_prev = next; X.delta_valid = true; X.delta_key = key; }
};

// what every stream call refuses beside its frame's own refusals; bound: the stream's
int check_stream_call(ycge_ctx *c, const char *fn, int32_t W, int32_t H, int32_t vx, int32_t vy, const uint8_t *out_stream, size_t capacity, const size_t *out_len,
                      unsigned long long &bound)
{
    if (!out_stream || !out_len) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (vx < 0 || vy < 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: viewport (%d, %d) (neither may be negative)", fn, vx, vy);
    if (!stream_bound(W, H, bound) || H > kMaxRows)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: the stream of %d x %d pixels may reach 2^32 bytes (offsets are 32-bit), or has more than %d rows", fn, W, H, kMaxRows);
    if (capacity < bound) return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (ycge_sixel_stream_bound)", fn, capacity, bound);
    return YCGE_OK;
}

// behind the synchronisation of a stream call: the host encoder on the planes read back (YCGE_SIXEL_HOST), or the device's stream.  prev:
// the call is a delta; info: 4 words or NULL
int finish_stream(ycge_ctx *c, SixelState &S, const char *fn, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, bool delta, unsigned long long bound,
                  uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *info)
{
    uint32_t words[4] = {1, 0, 0, 0};
    int rc;
    if (host_encoder_asked()) {
        const size_t n = (size_t)W * H;
        const uint8_t *cur = S.stage.data() + 5 * n;
        rc = delta ? sixel_encode_delta_host(cur + n, cur, W, H, vx, vy, out_stream, capacity, out_len, words) : sixel_encode_host(cur, W, H, vx, vy, clear, out_stream, capacity, out_len);
        if (rc != YCGE_OK) return c->fail(rc, "%s: the host encoder refused the frame's register plane", fn);
    } else {
        rc = deliver(c, S, fn, bound, out_stream, out_len, delta ? words : nullptr);
        if (rc != YCGE_OK) return rc;
    }
    if (info) std::memcpy(info, words, sizeof words);
    return YCGE_OK;
}

} // namespace

namespace ycge_host {

int sixel_frame_stream_delta(ycge_ctx *c, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream,
                             size_t capacity, size_t *out_len, uint32_t *out_info, float *out_top_bottom_sdr, ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_render_frame_sixel_delta";
    unsigned long long bound = 0;
    // (the order of ycge_render_frame_sixel's refusals: the stream's pointers and viewport, the frame, the bound)
    if (!out_stream || !out_len) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (viewport_x < 0 || viewport_y < 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: viewport (%d, %d) (neither may be negative)", fn, viewport_x, viewport_y);
    int rc = check_pixel_frame(c, fn, dither);
    if (rc == YCGE_OK) rc = check_stream_call(c, fn, c->hiW, c->hiH, viewport_x, viewport_y, out_stream, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const int32_t W = c->hiW, H = c->hiH;
    SixelState &S = c->sixel;
    SixelDeltaCall call(c, W, H, viewport_x, viewport_y, clear_screen != 0, keyframe != 0);
    DevBuf<uint8_t> &plane = S.held[call.next];
    if (plane.cap < (size_t)W * H) HIP_TRY(c, plane.alloc((size_t)W * H));
    rc = ensure_tables(c, c->chexels);
    if (rc == YCGE_OK && !host_encoder_asked()) rc = ensure_encoder(c, S, W, H, viewport_x, viewport_y, clear_screen != 0, bound, !call.keyframe);
    if (rc != YCGE_OK) return rc;
    const FrameOutputs::Pixels q{nullptr, nullptr, dither, true, viewport_x, viewport_y, clear_screen != 0, plane.p, call.prev()};
    FrameOutputs out(out_top_bottom_sdr);
    out.pixels = &q;
    rc = render_frame_sync(c, &out, st);          // (its stream synchronisation: the length has arrived)
    if (rc != YCGE_OK) return rc;
    c->chexels.delta_valid = false;               // (whatever the frame did to the state: the commit alone makes it valid)
    rc = finish_stream(c, S, fn, W, H, viewport_x, viewport_y, clear_screen, !call.keyframe, bound, out_stream, capacity, out_len, out_info);
    if (rc != YCGE_OK) return rc;
    call.commit();
    return YCGE_OK;
}

// the three Video mode calls.  The planes call: no stream.  keyframe < 0: ycge_video_blit_sixel, the full stream and an invalid delta state
// behind it; else ycge_video_blit_sixel_delta
static int video_pixels_call(ycge_ctx *c, const char *fn, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, float *out_sdr, uint8_t *out_rgba,
                             uint8_t *out_index, int32_t dither, bool stream, int32_t vx, int32_t vy, int32_t clear, int32_t keyframe, uint8_t *out_stream,
                             size_t capacity, size_t *out_len, uint32_t *out_info, int32_t pal_hold = -1, bool pal = false, uint8_t *out_palette = nullptr,
                             int32_t *out_count = nullptr)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    int rc = video_check_frame(c, fn, frame, src_w, src_h, bpp);
    if (rc != YCGE_OK) return rc;
    if (!stream && !out_sdr && !out_rgba && !out_index && !out_palette && !out_count)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: every destination is NULL (ask for at least one of sdr, rgba, index)", fn);
    if (dither < 0 || dither > 1) return c->fail(YCGE_ERR_INVALID_ARG, "%s: dither %d (0 or 1)", fn, dither);
    const int64_t W64 = (int64_t)c->fbW * c->ss, H64 = (int64_t)2 * c->fbH * c->ss;
    if (W64 * H64 > (int64_t)INT32_MAX / 2)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: a picture of %lld x %lld pixels (at most 2^30 pixels)", fn, (long long)W64, (long long)H64);
    const int32_t W = (int32_t)W64, H = (int32_t)H64;
    unsigned long long bound = 0;
    if (pal) { rc = check_palette_call(c, fn, stream, W, H, vx, vy, pal_hold, out_stream, capacity, out_len, bound); if (rc != YCGE_OK) return rc; }
    else if (stream) { rc = check_stream_call(c, fn, W, H, vx, vy, out_stream, capacity, out_len, bound); if (rc != YCGE_OK) return rc; }
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    SixelState &S = c->sixel;
    const size_t n = (size_t)W * H;
    const bool pal_pixels = pal && (stream || out_rgba || out_index || out_palette || out_count);          // (the SDR alone: ycge_video_blit's call)
    const bool pixels = stream || out_rgba || out_index || pal_pixels, delta = stream && keyframe >= 0;
    const bool pal_host = pal && stream && host_encoder_asked();
    bool pal_build = false;
    uint8_t *plane = nullptr;
    const uint8_t *prev = nullptr;
    bool key = true;
    int next = 0;
    if (delta) {
        SixelDeltaCall call(c, W, H, vx, vy, clear != 0, keyframe != 0);
        key = call.keyframe; next = call.next; prev = call.prev();
        if (S.held[next].cap < n) HIP_TRY(c, S.held[next].alloc(n));
        plane = S.held[next].p;
    } else if (pixels) {
        if (S.index.cap < n) HIP_TRY(c, S.index.alloc(n));
        plane = S.index.p;
    }
    if (pixels) {
        if ((out_rgba || pal_pixels) && S.rgba.cap < 4 * n) HIP_TRY(c, S.rgba.alloc(4 * n));
        rc = ensure_tables(c, c->chexels);
        if (rc == YCGE_OK && pal_pixels) rc = ensure_palette(c, S);
        if (rc == YCGE_OK && pal_pixels && stream && !pal_host) rc = ensure_encoder_palette(c, S, W, H, vx, vy, clear != 0, bound);
        if (rc == YCGE_OK && !pal && stream && !host_encoder_asked()) rc = ensure_encoder(c, S, W, H, vx, vy, clear != 0, bound, delta && !key);
        if (rc != YCGE_OK) return rc;
        if (pal_pixels) { pal_build = pal_hold == 0 || !S.pal_kept; S.pal_kept = false; }          // (kept again when the call has succeeded)
    }
    FrameOutputs::Pixels q{out_rgba, out_index, dither, stream, vx, vy, clear != 0, plane, prev};
    q.pal = pal_pixels ? (pal_build ? 2 : 1) : 0;
    FrameOutputs out(out_sdr);
    if (pixels) out.pixels = &q;
    const float *d_sdr = nullptr;
    rc = video_enqueue(c, c->stream, frame, src_w, src_h, bpp, c->fbW, c->fbH, c->ss, &d_sdr, nullptr, out_sdr != nullptr);
    if (rc == YCGE_OK && pixels) {
        const int e = ycge_launch_video_pixels(c->video.frame.p, src_w, src_h, bpp, c->fbW, c->fbH, c->ss, c->video.tables.p, c->chexels.tables.p, dither,
                                               (out_rgba || pal_pixels) ? S.rgba.p : nullptr, pal_pixels ? nullptr : plane, c->stream);
        if (e != 0) rc = c->fail(YCGE_ERR_DEVICE, "k_video_pixels launch failed: %s", hipGetErrorString((hipError_t)e));
        if (rc == YCGE_OK && pal_pixels && !pal_host) rc = launch_palette(c, S, S.rgba.p, W, H, pal_build, (stream || out_index) ? plane : nullptr, c->stream);
    }
    if (rc == YCGE_OK) rc = video_read_sdr(c, c->stream, d_sdr, out);
    if (rc == YCGE_OK && pixels) rc = planes_read_back(c, c->stream, out, W, H);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }          // (nothing of this call is queued when it returns)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    out.finish();
    if (pal_pixels) {
        if (pal_host) rc = palette_stream_on_host(c, S, fn, S.stage.data() + 5 * n, S.stage.data() + 9 * n, W, H, vx, vy, clear, pal_build, out_stream, capacity, out_len, out_palette, out_count);
        else if (stream) rc = deliver(c, S, fn, bound, out_stream, out_len);
        if (rc != YCGE_OK) return rc;
        if (!pal_host) palette_out(S, out_palette, out_count);
        S.pal_kept = true;
        if (stream) c->chexels.delta_valid = false;          // (the picture lies over the cells and over the cube's picture)
        return YCGE_OK;
    }
    if (!stream) return YCGE_OK;
    rc = finish_stream(c, S, fn, W, H, vx, vy, clear, delta && !key, bound, out_stream, capacity, out_len, out_info);
    if (rc != YCGE_OK) return rc;
    // (the picture lies over the terminal's cells: behind the plain call the next _delta call of any family is a keyframe; a delta call commits)
    c->chexels.delta_valid = false;
    if (delta) { S.held_prev = next; c->chexels.delta_valid = true; c->chexels.delta_key = ChexelState::DeltaKey{{SixelState::kSixelFamily, 0, 0, W, H, vx, vy, 0, 0, c->fbW, c->fbH}}; }
    return YCGE_OK;
}

int sixel_video_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, float *out_top_bottom_sdr, uint8_t *out_rgba, uint8_t *out_index,
                       int32_t dither)
{
    return video_pixels_call(c, "ycge_video_blit_pixels", frame, src_w, src_h, bpp, out_top_bottom_sdr, out_rgba, out_index, dither, false, 0, 0, 0, -1, nullptr, 0,
                             nullptr, nullptr);
}

int sixel_video_stream(ycge_ctx *c, const char *fn, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t viewport_x, int32_t viewport_y,
                       int32_t clear_screen, int32_t keyframe, int32_t dither, uint8_t *out_stream, size_t capacity, size_t *out_len, uint32_t *out_info,
                       float *out_top_bottom_sdr)
{
    return video_pixels_call(c, fn, frame, src_w, src_h, bpp, out_top_bottom_sdr, nullptr, nullptr, dither, true, viewport_x, viewport_y, clear_screen, keyframe,
                             out_stream, capacity, out_len, out_info);
}

int sixel_video_palette(ycge_ctx *c, const char *fn, bool stream, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t viewport_x, int32_t viewport_y,
                        int32_t clear_screen, int32_t hold, uint8_t *out_stream, size_t capacity, size_t *out_len, uint8_t *out_rgba, uint8_t *out_index,
                        uint8_t *out_palette, int32_t *out_count, float *out_top_bottom_sdr)
{
    return video_pixels_call(c, fn, frame, src_w, src_h, bpp, out_top_bottom_sdr, out_rgba, out_index, 0, stream, viewport_x, viewport_y, clear_screen, -1, out_stream,
                             capacity, out_len, nullptr, hold, true, out_palette, out_count);
}

// ---- the adaptive palette: the bound, the host functions, the frame call (stream or planes) and the two hooks

int sixel_palette_stream_bound(int32_t px_w, int32_t px_h, size_t *bytes)
{
    unsigned long long b = 0;
    if (!bytes || !palette_stream_bound(px_w, px_h, b)) return YCGE_ERR_INVALID_ARG;
    *bytes = (size_t)b;
    return YCGE_OK;
}

int sixel_palette_host(const uint8_t *rgba, int32_t W, int32_t H, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count)
{
    return ycge_sixel_host::palette(rgba, W, H, out_index, out_palette, out_pct, out_count);
}

int sixel_encode_palette_host(const uint8_t *index, const uint8_t *pct, int32_t count, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out,
                              size_t capacity, size_t *out_len)
{
    return ycge_sixel_host::encode_palette(index, pct, count, W, H, vx, vy, clear, out, capacity, out_len);
}

int sixel_frame_palette(ycge_ctx *c, const char *fn, bool stream, int32_t viewport_x, int32_t viewport_y, int32_t clear_screen, int32_t hold, uint8_t *out_stream,
                        size_t capacity, size_t *out_len, uint8_t *out_rgba, uint8_t *out_index, uint8_t *out_palette, int32_t *out_count, float *out_top_bottom_sdr,
                        ycge_frame_stats *st)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!stream && !out_top_bottom_sdr && !out_rgba && !out_index && !out_palette && !out_count)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: every destination is NULL (ask for at least one of sdr, rgba, index, palette, count)", fn);
    // (the order of ycge_render_frame_sixel's refusals: the stream's pointers and viewport, then hold, the frame, the bound)
    if (stream && (!out_stream || !out_len)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: out_stream and out_len must not be NULL", fn);
    if (stream && (viewport_x < 0 || viewport_y < 0)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: viewport (%d, %d) (neither may be negative)", fn, viewport_x, viewport_y);
    if (hold < 0 || hold > 1) return c->fail(YCGE_ERR_INVALID_ARG, "%s: hold %d (0 or 1)", fn, hold);
    int rc = check_pixel_frame(c, fn, 0);
    unsigned long long bound = 0;
    if (rc == YCGE_OK) rc = check_palette_call(c, fn, stream, c->hiW, c->hiH, viewport_x, viewport_y, hold, out_stream, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    FrameOutputs out(out_top_bottom_sdr);
    if (!stream && !out_rgba && !out_index && !out_palette && !out_count) return render_frame_sync(c, &out, st);          // (the SDR alone: ycge_render_frame's frame)
    rc = join_async(c);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    SixelState &S = c->sixel;
    const int32_t W = c->hiW, H = c->hiH;
    const size_t n = (size_t)W * H;
    const bool on_host = stream && host_encoder_asked();
    rc = ensure_planes(c, S, true);
    if (rc == YCGE_OK) rc = ensure_palette(c, S);
    if (rc == YCGE_OK && stream && !on_host) rc = ensure_encoder_palette(c, S, W, H, viewport_x, viewport_y, clear_screen != 0, bound);
    if (rc != YCGE_OK) return rc;
    const bool build = hold == 0 || !S.pal_kept;
    S.pal_kept = false;                            // (kept again when the call has succeeded)
    FrameOutputs::Pixels q{out_rgba, out_index, 0, stream, viewport_x, viewport_y, clear_screen != 0};
    q.pal = build ? 2 : 1;
    out.pixels = &q;
    rc = render_frame_sync(c, &out, st);          // (its stream synchronisation: the head, and with it the length, has arrived)
    if (rc != YCGE_OK) return rc;
    if (on_host) rc = palette_stream_on_host(c, S, fn, S.stage.data() + 5 * n, S.stage.data() + 9 * n, W, H, viewport_x, viewport_y, clear_screen, build, out_stream, capacity, out_len, out_palette, out_count);
    else if (stream) rc = deliver(c, S, fn, bound, out_stream, out_len);
    if (rc != YCGE_OK) return rc;
    if (!on_host) palette_out(S, out_palette, out_count);
    S.pal_kept = true;
    if (stream) c->chexels.delta_valid = false;          // (the picture lies over the cells and over the cube's picture: the next _delta call of any family is a keyframe)
    return YCGE_OK;
}

// test hooks: the palette stage alone (out == NULL) or the stage and the PAL encoder on a caller's RGBA plane of any W x H, with planes and
// encoder buffers of their own - but the context's kept palette, which `hold` reads and a success replaces as a _palette call does.  No
// frame or delta state is touched.  YCGE_SIXEL_HOST: the stream hook runs the host's functions
static int test_palette(ycge_ctx *c, const char *fn, const uint8_t *rgba, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, int32_t hold, uint8_t *out,
                        size_t capacity, size_t *out_len, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    const bool stream = out != nullptr || out_len != nullptr;
    if (!rgba || W <= 0 || H <= 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad arguments (%d x %d pixels)", fn, W, H);
    unsigned long long bound = 0;
    int rc = check_palette_call(c, fn, stream, W, H, vx, vy, hold, out, capacity, out_len, bound);
    if (rc != YCGE_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    SixelState &K = c->sixel;                      // (the kept palette alone)
    rc = ensure_palette(c, K);
    if (rc != YCGE_OK) return rc;
    const size_t n = (size_t)W * H;
    const bool build = hold == 0 || !K.pal_kept;
    K.pal_kept = false;
    if (stream && host_encoder_asked()) {
        std::vector<uint8_t> index(n);
        rc = palette_stream_on_host(c, K, fn, rgba, index.data(), W, H, vx, vy, clear, build, out, capacity, out_len, nullptr, nullptr);
        if (rc == YCGE_OK) K.pal_kept = true;
        return rc;
    }
    SixelState S;                                  // the encoder's buffers; the block is the context's
    DevBuf<uint8_t> planes;                        // the RGBA plane, the registers behind it
    HIP_TRY(c, planes.alloc(5 * n));
    if (stream) {
        rc = ensure_encoder_palette(c, S, W, H, vx, vy, clear != 0, bound);
        if (rc != YCGE_OK) return rc;
    }
    HIP_TRY(c, hipMemcpy(planes.p, rgba, 4 * n, hipMemcpyHostToDevice));
    rc = launch_palette(c, K, planes.p, W, H, build, planes.p + 4 * n, c->stream);
    if (rc == YCGE_OK && stream) {
        const size_t bands = (size_t)(H + 5) / 6, max_lines = bands * (size_t)(6 * (int64_t)W < 256 ? 6 * W : 256);
        const int e = ycge_launch_sixel_encode_palette(planes.p + 4 * n, W, H, S.last1.p, S.lines.p, S.line_bytes.p, (uint32_t)max_lines, S.meta.p, S.pal_prefix.p,
                                                       S.pal_prefix_bytes, K.pal_block.p + kPalDefs, reinterpret_cast<const uint32_t *>(K.pal_block.p + kPalDefsBytes),
                                                       S.stream.p, (uint32_t)bound, reinterpret_cast<unsigned long long *>(K.pal_block.p + kPalLength), c->compute_units,
                                                       c->stream);
        if (e != 0) rc = c->fail(YCGE_ERR_DEVICE, "the sixel encoder's launches failed: %s", hipGetErrorString((hipError_t)e));
    }
    if (rc == YCGE_OK) rc = copy_palette_head(c, K, c->stream);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stream) {
        const unsigned long long len = *static_cast<const unsigned long long *>(K.res_host.p);
        if (len > bound) return c->fail(YCGE_ERR_DEVICE, "%s: the device wrote a stream of %llu bytes, above its bound %llu", fn, len, bound);
        rc = copy_out(c, out, S.stream.p, (size_t)len);
        if (rc != YCGE_OK) return rc;
        *out_len = (size_t)len;
    }
    palette_out(K, out_palette, out_count, out_pct);
    if (out_index) { rc = copy_out(c, out_index, planes.p + 4 * n, n); if (rc != YCGE_OK) return rc; }
    K.pal_kept = true;
    return YCGE_OK;
}

int sixel_test_palette(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t hold, uint8_t *out_index, uint8_t *out_palette, uint8_t *out_pct, int32_t *out_count)
{
    return test_palette(c, "ycge_test_sixel_palette", rgba, W, H, 0, 0, 0, hold, nullptr, 0, nullptr, out_index, out_palette, out_pct, out_count);
}

int sixel_test_palette_stream(ycge_ctx *c, const uint8_t *rgba, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, int32_t hold, uint8_t *out, size_t capacity,
                              size_t *out_len)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (!out || !out_len) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_test_sixel_palette_stream: out and out_len must not be NULL");
    return test_palette(c, "ycge_test_sixel_palette_stream", rgba, W, H, vx, vy, clear, hold, out, capacity, out_len, nullptr, nullptr, nullptr, nullptr);
}

// test hook: the delta encoder's kernels alone on two caller's register planes of any W x H whose bound fits (values of 216 or more are
// refused here, on the host), with buffers of its own: nothing of the context's sixel or delta state is touched.  YCGE_SIXEL_HOST: the host encoder
int sixel_test_delta_stream(ycge_ctx *c, const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity,
                            size_t *out_len, uint32_t *out_info)
{
    if (!c) return YCGE_ERR_INVALID_ARG;
    static const char fn[] = "ycge_test_sixel_delta_stream";
    unsigned long long bound = 0;
    if (!prev || !index || !out || !out_len || vx < 0 || vy < 0 || !stream_bound(W, H, bound) || H > kMaxRows)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad arguments (%d x %d pixels at (%d, %d))", fn, W, H, vx, vy);
    if (capacity < bound) return c->fail(YCGE_ERR_INVALID_ARG, "%s: capacity %zu bytes is below the stream's bound %llu (ycge_sixel_stream_bound)", fn, capacity, bound);
    const size_t n = (size_t)W * H;
    for (size_t i = 0; i < n; i++)
        if (index[i] >= 216 || prev[i] >= 216) return c->fail(YCGE_ERR_INVALID_ARG, "%s: register %d / %d at pixel %zu (0..215)", fn, (int)prev[i], (int)index[i], i);
    if (host_encoder_asked()) return sixel_encode_delta_host(prev, index, W, H, vx, vy, out, capacity, out_len, out_info);
    HIP_TRY(c, hipSetDevice(c->device));
    SixelState S;
    DevBuf<uint8_t> planes;
    HIP_TRY(c, planes.alloc(2 * n));
    { const int rc = ensure_encoder(c, S, W, H, vx, vy, false, bound, true); if (rc != YCGE_OK) return rc; }
    HIP_TRY(c, hipMemcpy(planes.p, index, n, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(planes.p + n, prev, n, hipMemcpyHostToDevice));
    { const int rc = launch_encoder(c, S, planes.p, W, H, bound, c->stream, planes.p + n); if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; } }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t words[4] = {0, 0, 0, 0};
    const int rc = deliver(c, S, fn, bound, out, out_len, words);
    if (rc == YCGE_OK && out_info) std::memcpy(out_info, words, sizeof words);
    return rc;
}

} // namespace ycge_host
