// ycge_video.cpp - Video mode: VideoRenderer.TryFlipAndBlit (Renderer/VideoRenderer.cs:68-148) for a frame the host's IFrameReader
// shows (ycge_video_blit, ycge_video_blit_ansi; kernel: ycge_video.hip).
//
// A blit is: the frame's bytes up (through page-locked staging when the caller's array is pageable), one launch into an SDR array of
// this file's own, then what a ray-traced frame's presenters get - ycge_chexel.cpp's encode and read-back and ycge_ansi.cpp's stream on
// the same stream - and one synchronisation.  It needs no scene and touches nothing a ray-traced frame reads.  The entry points
// themselves stand beside the calls they mirror (ycge_chexel.cpp, ycge_ansi.cpp: their request guards are private to those files).
// The quadrant-glyph forms (ycge_video_blit_quadrants, _ansi_quad, _ansi_quad_delta) launch k_video_blit_quadrants instead, which writes the
// 2 x 2 sub-cell colours into ChexelState::quad_sdr beside the SDR; k_fit_quadrants and the quadrant streams then run as for a traced frame.
//
// The Lanczos weights are separable: they depend on the hi-res column alone or on the hi-res row alone.  The host computes them ONCE per
// geometry with the C library's sinf - the function MathF.Sin calls - in binary32, operation for operation as SampleSourceLanczos
// (:184-221) does, and the kernel reads two small tables (the pattern of SrgbTables in ycge_chexel.cpp).  The reference's bilinear
// fallback (:215) is taken only when a weight sum is <= 0; libm's sums lie in [0.994, 1.0000001], and the builder checks every one: a
// geometry that ever produced such a sum fails with YCGE_ERR_INTERNAL instead of showing other pixels.
#include "ycge_ctx.h"

#include <cmath>

namespace {

// Sinc (:160-166), LanczosKernel (:169-174) with a = LanczosA = 3; MathF.PI = 3.14159274f
float sinc(float x)
{
    x = std::fabs(x);
    if (x < 1e-6f) return 1.0f;
    const float pix = 3.14159274f * x;
    return sinf(pix) / pix;
}
float lanczos3(float x)
{
    x = std::fabs(x);
    if (x >= 3.0f) return 0.0f;
    return sinc(x) * sinc(x / 3.0f);
}

// :75-81
void geometry(int src_w, int src_h, int hiW, int hiH, float &scale, float &offX, float &offY)
{
    const float scaleX = (float)hiW / (float)src_w;
    const float scaleY = (float)hiH / (float)src_h;
    scale = scaleX < scaleY ? scaleX : scaleY;
    const float dstW = (float)src_w * scale;
    const float dstH = (float)src_h * scale;
    offX = 0.5f * ((float)hiW - dstW);
    offY = 0.5f * ((float)hiH - dstH);
}

// one axis: for each of n hi-res positions p, s = (p + 0.5f - off) / scale (:113-116), p0 = (int)floor(s) (:188), the six kernel values
// of the taps p0 - 2 .. p0 + 3 (:202-207) times 1 / their sum (:217-221).  False when a sum is <= 0 (the reference's bilinear case) or a
// source position lies beyond 2^30.
bool axis_table(int n, float off, float scale, int32_t *p0, float *w, int &bad)
{
    for (int p = 0; p < n; p++) {
        const float s = ((float)p + 0.5f - off) / scale;
        if (!(std::fabs(s) < 1073741824.0f)) { bad = p; return false; }        // ((int)floor(s) would not be an index any more)
        const int i0 = (int)std::floor(s);
        float k[6], sum = 0.0f;
        for (int i = 0, ix = i0 - 2; ix <= i0 + 3; ix++, i++) {
            k[i] = lanczos3(s - (float)ix);
            sum += k[i];
        }
        if (!(sum > 0.0f)) { bad = p; return false; }
        const float inv = 1.0f / sum;
        for (int i = 0; i < 6; i++) w[(size_t)p * 6 + i] = k[i] * inv;
        p0[p] = i0;
    }
    return true;
}

// what ycge_launch_video_blit reads: int32 x0[hiW], f32 wx[hiW][6], int32 y0[hiH], f32 wy[hiH][6]
int build_tables(int src_w, int src_h, int fbW, int fbH, int ss, std::vector<uint32_t> &words, float geom[3], std::string &msg)
{
    const int hiW = fbW * ss, hiH = fbH * 2 * ss;
    geometry(src_w, src_h, hiW, hiH, geom[0], geom[1], geom[2]);
    words.assign((size_t)7 * ((size_t)hiW + hiH), 0u);
    int32_t *x0 = reinterpret_cast<int32_t *>(words.data());
    float *wx = reinterpret_cast<float *>(words.data()) + hiW;
    int32_t *y0 = x0 + (size_t)7 * hiW;
    float *wy = wx + (size_t)6 * hiW + hiH;
    int bad = 0;
    const bool okx = axis_table(hiW, geom[1], geom[0], x0, wx, bad);
    if (!okx || !axis_table(hiH, geom[2], geom[0], y0, wy, bad)) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "video blit %d x %d -> %d x %d ss %d: the Lanczos weights of hi-res %s %d sum to <= 0 or its source position is beyond 2^30 "
                      "(the reference's bilinear fallback, VideoRenderer.cs:215, is not implemented on the device)", src_w, src_h, fbW, fbH, ss, okx ? "row" : "column", bad);
        msg = buf;
        return YCGE_ERR_INTERNAL;
    }
    return YCGE_OK;
}

bool geometry_ok(int fbW, int fbH, int ss)
{
    return fbW >= 1 && fbH >= 1 && ss >= 1 && ss <= 4096 && (int64_t)fbW * ss <= (int64_t)INT32_MAX / 8 && (int64_t)fbH * 2 * ss <= (int64_t)INT32_MAX / 8 &&
           (int64_t)fbW * fbH <= (int64_t)INT32_MAX / 2;
}

} // namespace

namespace ycge_host {

int video_check_frame(ycge_ctx *c, const char *fn, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp)
{
    if (!frame) return c->fail(YCGE_ERR_INVALID_ARG, "%s: frame is NULL", fn);
    if (src_w < 1 || src_h < 1) return c->fail(YCGE_ERR_INVALID_ARG, "%s: a source frame of %d x %d pixels (both must be positive)", fn, src_w, src_h);
    if (bpp != 3 && bpp != 4) return c->fail(YCGE_ERR_INVALID_ARG, "%s: %d bytes per pixel (3 = BGR, 4 = BGRA)", fn, bpp);
    if ((int64_t)src_w * src_h * bpp >= ((int64_t)1 << 31)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: a source frame of %d x %d x %d bytes reaches 2^31", fn, src_w, src_h, bpp);
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (!geometry_ok(c->fbW, c->fbH, c->ss)) return c->fail(YCGE_ERR_INVALID_ARG, "%s: the framebuffer %d x %d ss %d is beyond the blit's tables", fn, c->fbW, c->fbH, c->ss);
    return YCGE_OK;
}

// the tables of (src_w, src_h, fbW, fbH, ss) on the device: kept until another geometry is asked for
static int ensure_video_tables(ycge_ctx *c, VideoState &V, int src_w, int src_h, int fbW, int fbH, int ss)
{
    const int32_t key[5] = {src_w, src_h, fbW, fbH, ss};
    if (V.tables.p && std::memcmp(key, V.key, sizeof key) == 0) return YCGE_OK;
    std::vector<uint32_t> words;
    float geom[3];
    std::string msg;
    if (build_tables(src_w, src_h, fbW, fbH, ss, words, geom, msg) != YCGE_OK) return c->fail(YCGE_ERR_INTERNAL, "%s", msg.c_str());
    V.key[0] = 0;                                     // (no geometry while the buffer is rewritten)
    HIP_TRY(c, V.tables.reserve(words.size() * 4));
    HIP_TRY(c, hipMemcpy(V.tables.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
    std::memcpy(V.key, key, sizeof key);
    V.table_builds++;
    return YCGE_OK;
}

// quad_sdr (or NULL): the quadrant form - k_video_blit_quadrants writes the sub-cell colours there, fbW * fbH * 12 floats, beside the SDR
// (ss even: the caller's check_quadrant_call)
int video_enqueue(ycge_ctx *c, hipStream_t stream, const uint8_t *frame, int src_w, int src_h, int bpp, int fbW, int fbH, int ss, const float **d_sdr,
                  DevBuf<float> *quad_sdr, bool blit)
{
    VideoState &V = c->video;
    { const int rc = ensure_video_tables(c, V, src_w, src_h, fbW, fbH, ss); if (rc != YCGE_OK) return rc; }
    const size_t bytes = (size_t)src_w * src_h * bpp;
    HIP_TRY(c, V.frame.reserve(bytes));                // (DevBuf's padding takes the last 3-byte pixel's 32-bit load)
    HIP_TRY(c, V.sdr.reserve((size_t)fbW * fbH * 6));
    if (quad_sdr) HIP_TRY(c, quad_sdr->reserve((size_t)fbW * fbH * 12));
    const uint8_t *src = frame;
    if (!host_memory_is_page_locked(frame, bytes)) {   // the caller's array is its own again when the call returns: every blit ends synchronised
        HIP_TRY(c, V.stage.reserve(bytes));
        std::memcpy(V.stage.p, frame, bytes);
        src = V.stage.data();
    }
    HIP_TRY(c, hipMemcpyAsync(V.frame.p, src, bytes, hipMemcpyHostToDevice, stream));
    *d_sdr = V.sdr.p;
    if (!blit) return YCGE_OK;
    const int e = quad_sdr ? ycge_launch_video_blit_quadrants(V.frame.p, src_w, src_h, bpp, fbW, fbH, ss, V.tables.p, V.sdr.p, quad_sdr->p, stream)
                           : ycge_launch_video_blit(V.frame.p, src_w, src_h, bpp, fbW, fbH, ss, V.tables.p, V.sdr.p, stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_video_blit%s launch failed: %s", quad_sdr ? "_quadrants" : "", hipGetErrorString((hipError_t)e));
    *d_sdr = V.sdr.p;
    return YCGE_OK;
}

int video_read_sdr(ycge_ctx *c, hipStream_t stream, const float *d_sdr, FrameOutputs &out)
{
    if (!out.sdr) return YCGE_OK;
    const size_t sdr_bytes = (size_t)c->fbW * c->fbH * 6 * sizeof(float);
    float *target = out.sdr;
    if (!host_memory_is_page_locked(out.sdr, sdr_bytes)) {          // (finished on the host behind the stream: out.finish())
        HIP_TRY(c, c->out_stage.reserve(sdr_bytes));
        target = out.redirect(out.sdr, c->out_stage.p, sdr_bytes);
    }
    HIP_TRY(c, hipMemcpyAsync(target, d_sdr, sdr_bytes, hipMemcpyDeviceToHost, stream));
    return YCGE_OK;
}

int video_host_tables(int32_t src_w, int32_t src_h, int32_t fbW, int32_t fbH, int32_t ss, int32_t *x0, float *wx, int32_t *y0, float *wy, float *geom3)
{
    if (src_w < 1 || src_h < 1 || !geometry_ok(fbW, fbH, ss) || !x0 || !wx || !y0 || !wy || !geom3) return YCGE_ERR_INVALID_ARG;
    std::vector<uint32_t> words;
    std::string msg;
    const int rc = build_tables(src_w, src_h, fbW, fbH, ss, words, geom3, msg);
    if (rc != YCGE_OK) { g_create_error = msg; return rc; }
    const size_t hiW = (size_t)fbW * ss, hiH = (size_t)fbH * 2 * ss;
    std::memcpy(x0, words.data(), hiW * 4);
    std::memcpy(wx, words.data() + hiW, 6 * hiW * 4);
    std::memcpy(y0, words.data() + 7 * hiW, hiH * 4);
    std::memcpy(wy, words.data() + 7 * hiW + hiH, 6 * hiH * 4);
    return YCGE_OK;
}

// quad_out (or NULL): ycge_test_video_blit_quadrants - the quadrant form into a buffer of the hook's own, so the context's planes stay what they were
int video_test_blit(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t fbW, int32_t fbH, int32_t ss, float *sdr_out, float *quad_out)
{
    const char *fn = quad_out ? "ycge_test_video_blit_quadrants" : "ycge_test_video_blit";
    if (!frame || !sdr_out || src_w < 1 || src_h < 1 || (bpp != 3 && bpp != 4) || (int64_t)src_w * src_h * bpp >= ((int64_t)1 << 31) || !geometry_ok(fbW, fbH, ss))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad arguments (%d x %d x %d -> %d x %d ss %d)", fn, src_w, src_h, bpp, fbW, fbH, ss);
    if (quad_out && (ss < 2 || (ss & 1)))
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: super_sample %d (the quadrants halve a chexel's columns: it must be even)", fn, ss);
    { const int jr = join_async(c); if (jr != YCGE_OK) return jr; }
    HIP_TRY(c, hipSetDevice(c->device));
    const float *d_sdr = nullptr;
    DevBuf<float> quad;
    const int rc = video_enqueue(c, c->stream, frame, src_w, src_h, bpp, fbW, fbH, ss, &d_sdr, quad_out ? &quad : nullptr);
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int rs = copy_out(c, sdr_out, d_sdr, (size_t)fbW * fbH * 6 * sizeof(float));
    if (rs != YCGE_OK || !quad_out) return rs;
    return copy_out(c, quad_out, quad.p, (size_t)fbW * fbH * 12 * sizeof(float));
}

// test hook: k_video_pixels alone on a caller-given geometry, whatever the context's framebuffer is, with tables, frame and planes of its own
// on the context's device and stream: no video, sixel or delta state is touched.  Either output may be NULL, not both
int sixel_test_video_pixels(ycge_ctx *c, const uint8_t *frame, int32_t src_w, int32_t src_h, int32_t bpp, int32_t fbW, int32_t fbH, int32_t ss, int32_t dither,
                            uint8_t *out_rgba, uint8_t *out_index)
{
    static const char fn[] = "ycge_test_video_pixels";
    if (!frame || (!out_rgba && !out_index) || src_w < 1 || src_h < 1 || (bpp != 3 && bpp != 4) || (int64_t)src_w * src_h * bpp >= ((int64_t)1 << 31) ||
        !geometry_ok(fbW, fbH, ss) || (int64_t)fbW * fbH * 2 * ss * ss > ((int64_t)1 << 26) || dither < 0 || dither > 1)
        return c->fail(YCGE_ERR_INVALID_ARG, "%s: bad arguments (%d x %d x %d -> %d x %d ss %d, dither %d)", fn, src_w, src_h, bpp, fbW, fbH, ss, dither);
    HIP_TRY(c, hipSetDevice(c->device));
    { const int rc = ensure_tables(c, c->chexels); if (rc != YCGE_OK) return rc; }
    VideoState V;
    { const int rc = ensure_video_tables(c, V, src_w, src_h, fbW, fbH, ss); if (rc != YCGE_OK) return rc; }
    const size_t bytes = (size_t)src_w * src_h * bpp, n = (size_t)fbW * ss * fbH * 2 * ss;
    DevBuf<uint8_t> rgba, index;
    HIP_TRY(c, V.frame.reserve(bytes));                // (DevBuf's padding takes the last 3-byte pixel's 32-bit load)
    HIP_TRY(c, rgba.alloc(4 * n));
    HIP_TRY(c, index.alloc(n));
    HIP_TRY(c, hipMemcpy(V.frame.p, frame, bytes, hipMemcpyHostToDevice));
    const int e = ycge_launch_video_pixels(V.frame.p, src_w, src_h, bpp, fbW, fbH, ss, V.tables.p, c->chexels.tables.p, dither, out_rgba ? rgba.p : nullptr,
                                           out_index ? index.p : nullptr, c->stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "k_video_pixels launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = YCGE_OK;
    if (out_rgba) rc = copy_out(c, out_rgba, rgba.p, 4 * n);
    if (out_index && rc == YCGE_OK) rc = copy_out(c, out_index, index.p, n);
    return rc;
}

} // namespace ycge_host
