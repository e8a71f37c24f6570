// ycge_obj.cpp - OBJ meshes from file bytes: MeshLoader.FromObj (RayTracing/MeshLoader.cs:12-149) up to the float soup ycge_mesh.triangles
// takes (ycge_obj_parse_host, ycge_obj_parse, _read, _triangles, _release; kernels: ycge_obj.hip; the reading rules, the token routines
// and the host parser: ycge_obj.h), and MeshScenes.AddMeshAutoGround on the held OBJ (ycge_obj_ground_host, ycge_obj_ground,
// ycge_obj_triangles_auto_ground; kernels: ycge_obj_ground.hip; the contract and the host tail: ycge_obj.h).  The entry points themselves
// stand in ycge_host.cpp, thin wrappers behind the exception barrier.
//
// A parse is: the text up (through page-locked staging when the caller's array is pageable), the lines marked and counted, one read-back
// of the line count; the line table, each line's kind, two scans, one read-back of the position and triangle counts; the tokens parsed
// into positions and faces; the faces' indices checked and the box of the used vertices taken, one read-back of the verdicts.  Whatever
// the kernels decline - or the environment hands to the host - the host parser reads, and its positions and faces go up for the same last
// step: the held OBJ is the same arrays whoever parsed.  It needs no scene and touches nothing a frame reads.
#include "ycge_ctx.h"
#include "ycge_obj.h"

namespace {

// ObjHeader of ycge_obj.hip, as the host reads it back
struct ObjHeaderHost {
    unsigned long long err, bad_face;
    uint32_t decline, n_lines, n_positions, n_triangles;
    uint32_t used_box[6], tri_box[6];
};

// GroundHeader of ycge_obj_ground.hip, as the host reads it back
struct GroundHeaderHost {
    unsigned long long best;
    uint32_t decline, changed, n_components, n_used;
    uint32_t box[6];
    float sum[3], centroid[3];
    uint32_t pad[2];
};
static_assert(sizeof(ycge_obj_ground_info) == 64 && sizeof(ycge_obj::GroundInfo) == sizeof(ycge_obj_ground_info), "ycge_obj_ground_info is 64 bytes, and ycge_obj.h mirrors it");

float unordered(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// an ordered-integer box of the kernels -> min xyz, max xyz (nothing grew it: +inf, -inf, the reference's start values)
void decode_box(const uint32_t box[6], float mn[3], float mx[3])
{
    for (int a = 0; a < 3; a++) {
        const bool any = box[a] <= box[3 + a];
        mn[a] = any ? unordered(box[a]) : INFINITY;
        mx[a] = any ? unordered(box[3 + a]) : -INFINITY;
    }
}

void put_msg(char *msg, size_t msg_bytes, const std::string &text)
{
    if (msg && msg_bytes) std::snprintf(msg, msg_bytes, "%s", text.c_str());
}

} // namespace

namespace ycge_host {

int obj_parse_host(const uint8_t *text, size_t bytes, float *positions, int32_t *faces, ycge_obj_info *info, char *msg, size_t msg_bytes)
{
    if (info) std::memset(info, 0, sizeof *info);
    put_msg(msg, msg_bytes, "");
    if (!info) { put_msg(msg, msg_bytes, "ycge_obj_parse_host: info is NULL"); return YCGE_ERR_INVALID_ARG; }
    std::vector<float> pos;
    std::vector<int32_t> fc;
    int64_t n_lines = 0;
    std::string why;
    const int rc = ycge_obj::parse_host(text, bytes, pos, fc, n_lines, why);
    if (rc != YCGE_OK) { put_msg(msg, msg_bytes, why); return rc; }
    info->n_positions = (int32_t)(pos.size() / 3); info->n_triangles = (int32_t)(fc.size() / 3); info->n_lines = n_lines;
    if (positions) std::memcpy(positions, pos.data(), pos.size() * sizeof(float));
    if (faces) std::memcpy(faces, fc.data(), fc.size() * sizeof(int32_t));
    return YCGE_OK;
}

static void obj_drop(ycge_ctx *c)
{
    ObjState &O = c->obj;
    O.held = false;
    O.n_positions = O.n_triangles = O.on_device = 0; O.n_lines = 0;
    O.positions.release(); O.faces.release(); O.triangles.release(); O.header.release(); O.stage.release();
    O.ground_parent.release(); O.ground_count.release(); O.ground_first.release(); O.ground_terms.release(); O.ground_used.release(); O.ground_header.release();
}

static int read_header(ycge_ctx *c, ObjHeaderHost &h)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return copy_out(c, &h, c->obj.header.p, sizeof h);
}

// the text on the device: d_text is readable to the next multiple of 16 bytes (DevBuf's padding covers it)
static int upload_text(ycge_ctx *c, const uint8_t *text, size_t bytes, DevBuf<uint8_t> &d_text)
{
    HIP_TRY(c, d_text.alloc(bytes));
    if (host_memory_is_page_locked(text, bytes)) { HIP_TRY(c, hipMemcpyAsync(d_text.p, text, bytes, hipMemcpyHostToDevice, c->stream)); return YCGE_OK; }
    const size_t chunk = (size_t)32 << 20;
    HIP_TRY(c, c->obj.stage.reserve(bytes < chunk ? bytes : chunk));
    for (size_t off = 0; off < bytes; off += chunk) {
        const size_t n = bytes - off < chunk ? bytes - off : chunk;
        std::memcpy(c->obj.stage.p, text + off, n);
        HIP_TRY(c, hipMemcpyAsync(d_text.p + off, c->obj.stage.p, n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));          // (the one staging block is rewritten by the next chunk)
    }
    return YCGE_OK;
}

static int launch_failed(ycge_ctx *c, const char *what, int e) { return c->fail(YCGE_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString((hipError_t)e)); }

// The kernels' parse.  YCGE_OK with *declined = 0: positions and faces are on the device, counts in the state; *declined != 0: the host parser's
// file; a status: refused (the message is set) or failed.
static int parse_on_device(ycge_ctx *c, const uint8_t *text, size_t bytes, int *declined)
{
    ObjState &O = c->obj;
    *declined = 0;
    const uint32_t n = (uint32_t)bytes;
    const uint32_t first = n >= 3 && text[0] == 0xef && text[1] == 0xbb && text[2] == 0xbf ? 3u : 0u;
    DevBuf<uint8_t> d_text;
    DevBuf<uint32_t> tiles, line_start, add, block_pos, block_tri;
    { const int rc = upload_text(c, text, bytes, d_text); if (rc != YCGE_OK) return rc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto t0 = std::chrono::steady_clock::now();
    const size_t tile = ycge_launch_obj_sizes(1), per_block = ycge_launch_obj_sizes(2);
    HIP_TRY(c, O.header.reserve(ycge_launch_obj_sizes(0)));
    HIP_TRY(c, tiles.alloc((bytes + tile - 1) / tile));
    int e = ycge_launch_obj_count_lines(d_text.p, n, first, tiles.p, O.header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_obj_mark", e);
    ObjHeaderHost h;
    { const int rc = read_header(c, h); if (rc != YCGE_OK) return rc; }
    O.n_lines = h.n_lines;
    if (h.n_lines == 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s", ycge_obj::empty_text());          // (a byte-order mark and nothing else)
    const size_t n_blocks = ((size_t)h.n_lines + per_block - 1) / per_block;
    HIP_TRY(c, line_start.alloc(h.n_lines));
    HIP_TRY(c, add.alloc(h.n_lines));
    HIP_TRY(c, block_pos.alloc(n_blocks));
    HIP_TRY(c, block_tri.alloc(n_blocks));
    e = ycge_launch_obj_classify(d_text.p, n, first, tiles.p, line_start.p, h.n_lines, add.p, block_pos.p, block_tri.p, O.header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_obj_classify", e);
    { const int rc = read_header(c, h); if (rc != YCGE_OK) return rc; }
    O.last_us[0] = us_since(t0);
    if (h.decline) { *declined = (int)h.decline; return YCGE_OK; }
    t0 = std::chrono::steady_clock::now();
    const bool too_many = (int64_t)h.n_triangles > ycge_obj::kMaxTriangles;
    const bool writes = !too_many && h.n_positions > 0 && h.n_triangles > 0;          // otherwise the tokens are checked only: a malformed one is named first
    if (writes) {
        HIP_TRY(c, O.positions.reserve((size_t)3 * h.n_positions));
        HIP_TRY(c, O.faces.reserve((size_t)3 * h.n_triangles));
    }
    e = ycge_launch_obj_parse(d_text.p, n, line_start.p, h.n_lines, add.p, block_pos.p, block_tri.p, writes ? O.positions.p : nullptr, writes ? O.faces.p : nullptr,
                              h.n_positions, h.n_triangles, O.header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_obj_parse", e);
    { const int rc = read_header(c, h); if (rc != YCGE_OK) return rc; }
    O.last_us[1] = us_since(t0);
    if (h.decline) { *declined = (int)h.decline; return YCGE_OK; }
    if (h.err != ~0ull) {
        const int code = (int)(h.err & 0xffu);
        return c->fail(code == ycge_obj::NON_ASCII ? YCGE_ERR_UNSUPPORTED : YCGE_ERR_INVALID_ARG, "%s", ycge_obj::error_text((int64_t)(h.err >> 8), code).c_str());
    }
    if (too_many) return c->fail(YCGE_ERR_INVALID_ARG, "%s", ycge_obj::too_many_text());
    if (!writes) return c->fail(YCGE_ERR_INVALID_ARG, "%s", ycge_obj::empty_text());
    O.n_positions = (int32_t)h.n_positions; O.n_triangles = (int32_t)h.n_triangles;
    return YCGE_OK;
}

// positions and faces are on the device: the faces' indices checked, used[] marked, the box of the used vertices read back
static int finish_parse(ycge_ctx *c)
{
    ObjState &O = c->obj;
    const auto t0 = std::chrono::steady_clock::now();
    DevBuf<uint8_t> used;
    HIP_TRY(c, used.alloc((size_t)O.n_positions));
    HIP_TRY(c, O.header.reserve(ycge_launch_obj_sizes(0)));
    HIP_TRY(c, hipMemsetAsync(O.header.p, 0xff, 16, c->stream));          // (a host-parsed file: the header was never cleared)
    const int e = ycge_launch_obj_used_bounds(O.positions.p, O.faces.p, (uint32_t)O.n_positions, (uint32_t)O.n_triangles, used.p, O.header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_obj_used", e);
    ObjHeaderHost h;
    { const int rc = read_header(c, h); if (rc != YCGE_OK) return rc; }
    O.last_us[1] += us_since(t0);
    if (h.bad_face != ~0ull) return c->fail(YCGE_ERR_INVALID_ARG, "%s", ycge_obj::range_text((int64_t)h.bad_face, O.n_positions).c_str());
    decode_box(h.used_box, O.used_min, O.used_max);
    return YCGE_OK;
}

int obj_parse(ycge_ctx *c, const uint8_t *text, size_t bytes, ycge_obj_info *info)
{
    if (info) std::memset(info, 0, sizeof *info);
    if (!info) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_obj_parse: info is NULL");
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    { std::string why; const int rc = ycge_obj::check_text(text, bytes, why); if (rc != YCGE_OK) return c->fail(rc, "%s", why.c_str()); }
    { const int rc = join_async(c); if (rc != YCGE_OK) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    ObjState &O = c->obj;
    obj_drop(c);
    O.last_us[0] = O.last_us[1] = 0.0;
    int declined = c->knobs.obj_host ? (int)ycge_obj::DECLINE_ENV_HOST : (long long)bytes < c->knobs.obj_device_min ? (int)ycge_obj::DECLINE_BELOW_MIN : 0;
    int rc = YCGE_OK;
    if (!declined) rc = parse_on_device(c, text, bytes, &declined);
    if (rc == YCGE_OK && declined) {
        std::vector<float> pos;
        std::vector<int32_t> fc;
        std::string why;
        rc = ycge_obj::parse_host(text, bytes, pos, fc, O.n_lines, why);
        if (rc != YCGE_OK) (void)c->fail(rc, "%s", why.c_str());
        else {
            O.n_positions = (int32_t)(pos.size() / 3); O.n_triangles = (int32_t)(fc.size() / 3);
            hipError_t he = O.positions.upload(pos);
            if (he == hipSuccess) he = O.faces.upload(fc);
            if (he != hipSuccess) rc = c->fail(he == hipErrorOutOfMemory ? YCGE_ERR_OUT_OF_MEMORY : YCGE_ERR_DEVICE, "OBJ upload failed: %s", hipGetErrorString(he));
        }
    }
    if (rc == YCGE_OK) rc = finish_parse(c);
    O.stage.release();
    O.last_decline = declined;
    if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); obj_drop(c); return rc; }          // (nothing is held)
    O.on_device = declined ? 0 : 1;
    (declined ? O.host_parses : O.device_parses)++;
    O.held = true;
    info->n_positions = O.n_positions; info->n_triangles = O.n_triangles; info->n_lines = O.n_lines; info->on_device = O.on_device;
    return YCGE_OK;
}

static int obj_held(ycge_ctx *c, const char *fn)
{
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (!c->obj.held) return c->fail(YCGE_ERR_INVALID_ARG, "%s: the context holds no parsed OBJ (ycge_obj_parse first)", fn);
    { const int rc = join_async(c); if (rc != YCGE_OK) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    return YCGE_OK;
}

int obj_read(ycge_ctx *c, float *positions, int32_t *faces)
{
    { const int rc = obj_held(c, "ycge_obj_read"); if (rc != YCGE_OK) return rc; }
    const ObjState &O = c->obj;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int rc = YCGE_OK;
    if (positions) rc = copy_out(c, positions, O.positions.p, (size_t)3 * O.n_positions * sizeof(float));
    if (faces && rc == YCGE_OK) rc = copy_out(c, faces, O.faces.p, (size_t)3 * O.n_triangles * sizeof(int32_t));
    return rc;
}

// the placed soup of the held OBJ into O.triangles on the device (k_obj_triangles), its box into out_bounds (or NULL)
static int obj_triangles_on_device(ycge_ctx *c, int32_t normalize, float target_size, float scale, const float translate[3], float out_bounds[6])
{
    ObjState &O = c->obj;
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const float *t = translate ? translate : zero;
    // NormalizeAllUsedVertices (MeshLoader.cs:127-139)
    const float *mn = O.used_min, *mx = O.used_max;
    bool norm = normalize != 0;
    for (int a = 0; a < 3; a++) if (std::isinf(mn[a]) || std::isinf(mx[a])) norm = false;
    float ctr[3] = {0.0f, 0.0f, 0.0f}, s = 1.0f;
    if (norm) {
        for (int a = 0; a < 3; a++) ctr[a] = (mn[a] + mx[a]) * 0.5f;
        const float rx = mx[0] - mn[0], ry = mx[1] - mn[1], rz = mx[2] - mn[2];
        float max_extent = rx;
        if (ry > max_extent) max_extent = ry;
        if (rz > max_extent) max_extent = rz;
        if (max_extent <= 0.0f) max_extent = 1.0f;
        s = target_size / max_extent;
    }
    const bool transform = scale != 1.0f || t[0] != 0.0f || t[1] != 0.0f || t[2] != 0.0f;          // (:66)
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(c, O.triangles.reserve((size_t)9 * O.n_triangles));
    const int e = ycge_launch_obj_triangles(O.positions.p, O.faces.p, (uint32_t)O.n_triangles, norm ? 1 : 0, ctr, s, transform ? 1 : 0, scale, t, O.triangles.p, O.header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_obj_triangles", e);
    ObjHeaderHost h;
    { const int rc = read_header(c, h); if (rc != YCGE_OK) return rc; }
    O.last_us[2] = us_since(t0);
    if (out_bounds) decode_box(h.tri_box, out_bounds, out_bounds + 3);
    return YCGE_OK;
}

int obj_triangles(ycge_ctx *c, int32_t normalize, float target_size, float scale, const float translate[3], float *out_triangles, float out_bounds[6])
{
    { const int rc = obj_held(c, "ycge_obj_triangles"); if (rc != YCGE_OK) return rc; }
    if (!out_triangles) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_obj_triangles: out_triangles is NULL");
    { const int rc = obj_triangles_on_device(c, normalize, target_size, scale, translate, out_bounds); if (rc != YCGE_OK) return rc; }
    return copy_out(c, out_triangles, c->obj.triangles.p, (size_t)9 * c->obj.n_triangles * sizeof(float));
}

int obj_release(ycge_ctx *c)
{
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    { const int rc = join_async(c); if (rc != YCGE_OK) return rc; }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    obj_drop(c);
    return YCGE_OK;
}

int obj_stats(ycge_ctx *c, int64_t *out6)
{
    if (!out6) return YCGE_ERR_INVALID_ARG;
    if (!c) {
        Knobs knobs;
        knobs.read();
        out6[0] = (int64_t)ycge_launch_obj_sizes(1); out6[1] = (int64_t)ycge_launch_obj_sizes(2); out6[2] = (int64_t)ycge_launch_obj_sizes(3);
        out6[3] = knobs.obj_device_min; out6[4] = knobs.obj_host ? 1 : 0; out6[5] = 0;
        return YCGE_ERR_INVALID_ARG;
    }
    const ObjState &O = c->obj;
    out6[0] = O.device_parses; out6[1] = O.host_parses; out6[2] = O.last_decline;
    for (int a = 0; a < 3; a++) out6[3 + a] = (int64_t)O.last_us[a];
    return YCGE_OK;
}

int obj_ground_host(const float *positions, int32_t n_positions, const int32_t *faces, int32_t n_triangles, ycge_obj_ground_info *out)
{
    if (!out) return YCGE_ERR_INVALID_ARG;
    ycge_obj::GroundInfo g;
    const int rc = ycge_obj::ground_host(positions, n_positions, faces, n_triangles, g);
    std::memcpy(out, &g, sizeof g);
    return rc;
}

// The kernels' tail.  YCGE_OK with *declined = 0: *out is filled; *declined != 0: the host tail's OBJ; a status: failed.
static int ground_on_device(ycge_ctx *c, ycge_obj_ground_info *out, int *declined)
{
    ObjState &O = c->obj;
    *declined = 0;
    const uint32_t nv = (uint32_t)O.n_positions, nf = (uint32_t)O.n_triangles;
    const uint32_t chunk = (uint32_t)ycge_launch_obj_ground_sizes(1), padded = (nf + chunk - 1u) / chunk * chunk;
    const int round_cap = (int)ycge_launch_obj_ground_sizes(2);
    const bool phases = c->knobs.obj_ground_phases;          // a stream synchronise behind every phase: what each one costs
    for (double &u : O.ground_phase_us) u = 0.0;
    HIP_TRY(c, O.ground_header.reserve(ycge_launch_obj_ground_sizes(0)));
    HIP_TRY(c, O.ground_parent.reserve(nv));
    HIP_TRY(c, O.ground_count.reserve(nv));
    HIP_TRY(c, O.ground_first.reserve(nv));
    HIP_TRY(c, O.ground_used.reserve(nv));
    HIP_TRY(c, O.ground_terms.reserve((size_t)3 * padded));
    GroundHeaderHost h;
    auto read_back = [&]() -> int {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return copy_out(c, &h, O.ground_header.p, sizeof h);
    };
    auto t0 = std::chrono::steady_clock::now();
    auto phase_done = [&](int k) -> int {
        if (!phases) return YCGE_OK;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        O.ground_phase_us[k] = us_since(t0);
        t0 = std::chrono::steady_clock::now();
        return YCGE_OK;
    };
    // labelling: the first round does the work, every later one checks it across a launch boundary; the round that hooks nothing ends it
    int rounds = 0;
    for (;;) {
        const int e = ycge_launch_obj_ground_round(O.faces.p, nf, nv, O.ground_parent.p, rounds == 0 ? 1 : 0, O.ground_header.p, c->stream);
        if (e != 0) return launch_failed(c, "k_ground_hook", e);
        if (++rounds == 1) continue;
        { const int rc = read_back(); if (rc != YCGE_OK) return rc; }
        if (h.decline) break;
        if (!h.changed) break;
        if (rounds >= round_cap) { h.decline = (uint32_t)ycge_obj::GROUND_DECLINE_ROUND_CAP; break; }
    }
    O.ground_rounds = rounds;
    if (h.decline) { *declined = (int)h.decline; return YCGE_OK; }
    { const int rc = phase_done(0); if (rc != YCGE_OK) return rc; }
    int e = ycge_launch_obj_ground_select(O.faces.p, nf, nv, O.ground_parent.p, O.ground_count.p, O.ground_first.p, O.ground_header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_ground_count", e);
    { const int rc = phase_done(1); if (rc != YCGE_OK) return rc; }
    e = ycge_launch_obj_ground_terms(O.positions.p, O.faces.p, nf, nv, O.ground_parent.p, O.ground_terms.p, padded, O.ground_used.p, O.ground_header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_ground_terms", e);
    { const int rc = phase_done(2); if (rc != YCGE_OK) return rc; }
    e = ycge_launch_obj_ground_sum(O.ground_terms.p, padded, O.ground_header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_ground_sum", e);
    { const int rc = phase_done(3); if (rc != YCGE_OK) return rc; }
    e = ycge_launch_obj_ground_bounds(O.positions.p, nv, O.ground_used.p, O.ground_header.p, c->stream);
    if (e != 0) return launch_failed(c, "k_ground_bounds", e);
    { const int rc = read_back(); if (rc != YCGE_OK) return rc; }
    if (phases) O.ground_phase_us[4] = us_since(t0);
    ycge_obj::GroundInfo g;
    std::memset(&g, 0, sizeof g);
    float rmin[3], rmax[3];
    decode_box(h.box, rmin, rmax);
    for (int a = 0; a < 3; a++) g.centroid[a] = h.centroid[a];
    ycge_obj::ground_normalise(rmin, rmax, g);
    g.n_components = (int32_t)h.n_components; g.component_faces = (int32_t)(h.best >> 32); g.component_vertices = (int32_t)h.n_used;
    g.first_face = (int32_t)~(uint32_t)h.best; g.on_device = 1;
    std::memcpy(out, &g, sizeof g);
    return YCGE_OK;
}

int obj_ground(ycge_ctx *c, ycge_obj_ground_info *out)
{
    if (out) std::memset(out, 0, sizeof *out);
    { const int rc = obj_held(c, "ycge_obj_ground"); if (rc != YCGE_OK) return rc; }
    if (!out) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_obj_ground: out is NULL");
    ObjState &O = c->obj;
    const auto t0 = std::chrono::steady_clock::now();
    int declined = c->knobs.obj_ground_host ? (int)ycge_obj::GROUND_DECLINE_ENV_HOST : (long long)O.n_triangles < c->knobs.obj_ground_device_min ? (int)ycge_obj::GROUND_DECLINE_BELOW_MIN : 0;
    O.ground_rounds = 0;
    if (!declined) {
        const int rc = ground_on_device(c, out, &declined);
        if (rc != YCGE_OK) { (void)hipStreamSynchronize(c->stream); return rc; }
    }
    if (declined) {          // the host tail, on the held arrays
        std::vector<float> pos((size_t)3 * O.n_positions);
        std::vector<int32_t> fc((size_t)3 * O.n_triangles);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        { const int rc = copy_out(c, pos.data(), O.positions.p, pos.size() * sizeof(float)); if (rc != YCGE_OK) return rc; }
        { const int rc = copy_out(c, fc.data(), O.faces.p, fc.size() * sizeof(int32_t)); if (rc != YCGE_OK) return rc; }
        const int rc = obj_ground_host(pos.data(), O.n_positions, fc.data(), O.n_triangles, out);
        if (rc != YCGE_OK) return c->fail(rc, "ycge_obj_ground: the host tail refused the held OBJ");
    }
    O.ground_last_decline = declined;
    (declined ? O.ground_host_tails : O.ground_device_tails)++;
    O.ground_last_us = us_since(t0);
    return YCGE_OK;
}

// AddMeshAutoGround's placement of the held OBJ (the tail, then the soup on the device)
static int obj_auto_ground_on_device(ycge_ctx *c, float scale, const float target[3], float out_bounds[6], ycge_obj_ground_info *out_info)
{
    ycge_obj_ground_info g;
    { const int rc = obj_ground(c, &g); if (rc != YCGE_OK) return rc; }
    if (out_info) *out_info = g;
    // AddMeshAutoGround (MeshScenes.cs:180-183): each operation rounded to binary32 (this file is compiled without contraction)
    const float lifted = g.min[1] * scale;
    const float y_translate = (target[1] - lifted) + 0.01f;
    const float translate[3] = {target[0], y_translate, target[2]};
    return obj_triangles_on_device(c, 1, 1.0f, scale, translate, out_bounds);
}

int obj_triangles_auto_ground(ycge_ctx *c, float scale, const float target[3], float *out_triangles, float out_bounds[6], ycge_obj_ground_info *out_info)
{
    if (out_info) std::memset(out_info, 0, sizeof *out_info);
    { const int rc = obj_held(c, "ycge_obj_triangles_auto_ground"); if (rc != YCGE_OK) return rc; }
    if (!out_triangles || !target) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_obj_triangles_auto_ground: %s is NULL", out_triangles ? "target" : "out_triangles");
    { const int rc = obj_auto_ground_on_device(c, scale, target, out_bounds, out_info); if (rc != YCGE_OK) return rc; }
    return copy_out(c, out_triangles, c->obj.triangles.p, (size_t)9 * c->obj.n_triangles * sizeof(float));
}

// ycge_scene_attach_obj_mesh: the placed soup stays where k_obj_triangles wrote it and goes to the tree builder from there (ycge_mesh_pool.cpp)
int obj_attach_mesh(ycge_ctx *c, int32_t auto_ground, int32_t normalize, float target_size, float scale, const float translate_or_target[3], int32_t material,
                    int32_t *out_mesh_index, float out_bounds[6])
{
    { const int rc = obj_held(c, "ycge_scene_attach_obj_mesh"); if (rc != YCGE_OK) return rc; }
    if (!out_mesh_index || (auto_ground && !translate_or_target))
        return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_attach_obj_mesh: %s is NULL", out_mesh_index ? "the target" : "out_mesh_index");
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "no scene uploaded");
    if (material < 0 || material >= c->n_materials) return c->fail(YCGE_ERR_INVALID_ARG, "mesh 0: material out of range");
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    const int prc = auto_ground ? obj_auto_ground_on_device(c, scale, translate_or_target, bounds, nullptr)
                                : obj_triangles_on_device(c, normalize, target_size, scale, translate_or_target, bounds);
    if (prc != YCGE_OK) return prc;
    int32_t index = -1;
    const int rc = scene_attach_device_soup(c, c->obj.triangles.p, c->obj.n_triangles, material, &index);
    if (rc != YCGE_OK) return rc;
    *out_mesh_index = index;
    if (out_bounds) for (int a = 0; a < 6; a++) out_bounds[a] = bounds[a];
    return YCGE_OK;
}

int obj_ground_stats(ycge_ctx *c, int64_t *out6)
{
    if (!out6) return YCGE_ERR_INVALID_ARG;
    if (!c) {
        Knobs knobs;
        knobs.read();
        out6[0] = (int64_t)ycge_launch_obj_ground_sizes(1); out6[1] = (int64_t)ycge_launch_obj_ground_sizes(2); out6[2] = YCGE_OBJ_GROUND_DEVICE_MIN_DEFAULT;
        out6[3] = knobs.obj_ground_device_min; out6[4] = knobs.obj_ground_host ? 1 : 0; out6[5] = 0;
        return YCGE_ERR_INVALID_ARG;
    }
    const ObjState &O = c->obj;
    out6[0] = O.ground_device_tails; out6[1] = O.ground_host_tails; out6[2] = O.ground_last_decline; out6[3] = O.ground_rounds;
    out6[4] = 0;          // (no chunked sum is built: nothing falls back)
    out6[5] = (int64_t)O.ground_last_us;
    return YCGE_OK;
}

int obj_ground_phases(ycge_ctx *c, int64_t *out5)
{
    if (!c || !out5) return YCGE_ERR_INVALID_ARG;
    for (int a = 0; a < 5; a++) out5[a] = (int64_t)c->obj.ground_phase_us[a];
    return YCGE_OK;
}

} // namespace ycge_host
