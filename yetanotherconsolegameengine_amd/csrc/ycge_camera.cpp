// ycge_camera.cpp - VolumeScene's camera physics as one call a tick (ycge_volume_camera_tick; kernel: ycge_camera.hip; the stepper both
// sides run: ycge_camera_physics.h).
//
// The device route stages {body, world, moves} up through page-locked memory, waits for the device work of the last scene change
// (scene_ev, as a query does), launches k_camera_tick - one wavefront that runs the whole chain of rays and its control - reads the
// kernel's one record back and synchronises the query stream: one launch, one read-back, one synchronise.  It runs on the query stream
// with buffers of its own, so it waits for no frame in flight and writes nothing a frame reads.  *body and *info are written from the
// record on success only.  YCGE_CAMERA_HOST=1 runs the same stepper here, each window one batch of the scene queries' own run.
//
// ycge_volume_bodies_tick is the same for n independent bodies, each with its own shape (ycge_body_shape): one staged copy up, one launch
// of k_bodies_tick - a workgroup of one wavefront a body - one copy back, one synchronise; a body that reaches a cap keeps its state and
// says so in its result record, the others commit.  Its host route gathers the next window of every running body into one query batch.
//
// ycge_test_camera_tick_host and ycge_test_bodies_tick_host (include/ycge_hooks.h) are the stepper over a caller's Scene.Hit: no context,
// no device.  With -DYCGE_CAMERA_HOOK_ONLY this file is those hooks alone and needs no HIP (a stand-alone sanitizer build of the stepper).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ycge_camera_physics.h"
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wcomment"
#include "../../include/ycge_hooks.h"
#pragma GCC diagnostic pop
#ifndef YCGE_CAMERA_HOOK_ONLY
#include "ycge_ctx.h"
#endif

namespace {

using namespace ycge_cam;

// the refusals and the result of a tick, shared by the export and the hook: text into msg, the status code back
int refuse_text(char *msg, size_t msg_bytes, const char *fn, const char *why, int32_t bad_move)
{
    if (msg && msg_bytes) {
        if (bad_move >= 0) snprintf(msg, msg_bytes, "%s: move %d: %s", fn, bad_move, why);
        else snprintf(msg, msg_bytes, "%s: %s", fn, why);
    }
    return YCGE_ERR_INVALID_ARG;
}
int status_text(char *msg, size_t msg_bytes, const char *fn, int status, int32_t bad_move)
{
    if (msg && msg_bytes) {
        if (bad_move >= 0) snprintf(msg, msg_bytes, "%s: move %d: %s", fn, bad_move, cam_status_text(status));
        else snprintf(msg, msg_bytes, "%s: %s", fn, cam_status_text(status));
    }
    return YCGE_ERR_UNSUPPORTED;
}

const ycge_body_shape kDefaultShape = YCGE_BODY_SHAPE_DEFAULT;

// a begun tick to its end over a caller's Scene.Hit
void run_over_callback(Tick &t, ycge_camera_hit_fn hit, void *user, int32_t windowed)
{
    cam_run_host(t, [&](const Ray *rays, int n, Hit *hits) {
        for (int k = 0; k < n; k++) {
            const Ray &r = rays[k];
            const float ray[8] = {r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], r.tmin, r.tmax};
            float rec[7] = {0, 0, 0, 0, 0, 0, 0};
            hits[k].hit = hit(user, ray, rec) != 0 ? 1 : 0;
            hits[k].t = rec[0]; hits[k].nx = rec[4]; hits[k].ny = rec[5]; hits[k].nz = rec[6];
        }
        return 0;
    }, windowed ? kMaxWindow : 1);
}

// ---- many bodies a tick: what ycge_volume_bodies_tick and ycge_test_bodies_tick_host share
// what a batch is refused for before any work, the text into msg ("fn: body 7: move 2: why"): YCGE_OK, or YCGE_ERR_INVALID_ARG
int bodies_refusal(char *msg, size_t msg_bytes, const char *fn, const ycge_camera_body *bodies, const ycge_body_shape *shapes, int32_t n,
                   const ycge_camera_world *world, const ycge_camera_move *moves, const int32_t *move_first, float dt_ms, const ycge_body_result *results)
{
    auto refuse = [&](int32_t body, int32_t move, const char *why) {
        if (msg && msg_bytes) {
            if (body >= 0 && move >= 0) snprintf(msg, msg_bytes, "%s: body %d: move %d: %s", fn, body, move, why);
            else if (body >= 0) snprintf(msg, msg_bytes, "%s: body %d: %s", fn, body, why);
            else snprintf(msg, msg_bytes, "%s: %s", fn, why);
        }
        return (int)YCGE_ERR_INVALID_ARG;
    };
    if (n < 0 || n > YCGE_BODIES_MAX) return refuse(-1, -1, "n outside 0..YCGE_BODIES_MAX (4096)");
    if (n == 0) return YCGE_OK;
    if (!bodies || !world || !results || !move_first) return refuse(-1, -1, "NULL bodies, world, results or move_first with n > 0");
    if (!isfinite(world->world_height) || !isfinite(world->water_level) || !isfinite(world->voxel_size_y)) return refuse(-1, -1, "a field of the world is not finite");
    if (!isfinite(dt_ms)) return refuse(-1, -1, "delta_time_ms is not finite");
    if (move_first[0] != 0) return refuse(0, -1, "move_first[0] is not 0");
    for (int32_t i = 0; i < n; i++) {
        if (move_first[i + 1] < move_first[i]) return refuse(i, -1, "move_first decreases");
        if (move_first[i + 1] - move_first[i] > YCGE_CAMERA_MAX_MOVES) return refuse(i, -1, "more than YCGE_CAMERA_MAX_MOVES (32) moves");
        if (move_first[i + 1] > move_first[i] && !moves) return refuse(i, -1, "NULL moves while the body has moves");
    }
    for (int32_t i = 0; i < n; i++) {
        const int32_t first = move_first[i], count = move_first[i + 1] - first;
        int32_t bad = -1;
        if (const char *why = cam_refusal(&bodies[i], world, count > 0 ? moves + first : nullptr, count, dt_ms, &bad)) return refuse(i, bad, why);
        if (shapes)
            if (const char *why = cam_shape_refusal(shapes[i])) return refuse(i, -1, why);
    }
    return YCGE_OK;
}
void begin_body(Tick &t, int32_t i, const ycge_camera_body *bodies, const ycge_body_shape *shapes, const ycge_camera_world *world,
                const ycge_camera_move *moves, const int32_t *move_first, float dt_ms, int32_t run_update)
{
    const int32_t first = move_first[i], count = move_first[i + 1] - first;
    cam_begin(t, bodies[i], shapes ? shapes[i] : kDefaultShape, *world, count > 0 ? moves + first : nullptr, count, dt_ms, run_update);
}
// a finished tick into the caller's arrays: the body and its info on status 0 only
void commit_body(int32_t i, const ycge_camera_body &body, const ycge_camera_tick_info &tick_info, int32_t status, int32_t bad_move, ycge_camera_body *bodies,
                 ycge_body_result *results, ycge_camera_tick_info *info)
{
    results[i].status = status;
    results[i].bad_move = status == ST_OK ? -1 : bad_move;
    if (status != ST_OK) return;
    bodies[i] = body;
    if (info) info[i] = tick_info;
}

} // namespace

extern "C" int ycge_test_bodies_tick_host(ycge_camera_body *bodies, const ycge_body_shape *shapes, int32_t n, const ycge_camera_world *world,
                                          const ycge_camera_move *moves, const int32_t *move_first, float delta_time_ms, int32_t run_update,
                                          ycge_body_result *results, ycge_camera_tick_info *info, ycge_camera_hit_fn hit, void *user, int32_t windowed,
                                          char *msg, size_t msg_bytes)
try {
    const char *fn = "ycge_test_bodies_tick_host";
    const int rc = bodies_refusal(msg, msg_bytes, fn, bodies, shapes, n, world, moves, move_first, delta_time_ms, results);
    if (rc != YCGE_OK) return rc;
    if (!hit) return refuse_text(msg, msg_bytes, fn, "NULL hit callback", -1);
    for (int32_t i = 0; i < n; i++) {
        Tick t;
        begin_body(t, i, bodies, shapes, world, moves, move_first, delta_time_ms, run_update);
        run_over_callback(t, hit, user, windowed);
        commit_body(i, t.b, t.info, t.status, t.bad_move, bodies, results, info);
    }
    return YCGE_OK;
}
catch (...) { return YCGE_ERR_INTERNAL; }

extern "C" int ycge_test_camera_tick_host(ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves, int32_t n_moves,
                                          float delta_time_ms, int32_t run_update, ycge_camera_tick_info *info, ycge_camera_hit_fn hit, void *user,
                                          int32_t windowed, char *msg, size_t msg_bytes)
try {
    const char *fn = "ycge_test_camera_tick_host";
    int32_t bad = -1;
    if (const char *why = cam_refusal(body, world, moves, n_moves, delta_time_ms, &bad)) return refuse_text(msg, msg_bytes, fn, why, bad);
    if (!hit) return refuse_text(msg, msg_bytes, fn, "NULL hit callback", -1);
    Tick t;
    cam_begin(t, *body, kDefaultShape, *world, moves, n_moves, delta_time_ms, run_update);
    run_over_callback(t, hit, user, windowed);
    if (t.status != ST_OK) return status_text(msg, msg_bytes, fn, t.status, t.bad_move);
    *body = t.b;
    if (info) *info = t.info;
    return YCGE_OK;
}
catch (...) { return YCGE_ERR_INTERNAL; }

#ifndef YCGE_CAMERA_HOOK_ONLY

namespace ycge_host {
namespace {

// the stepper on the host, a window a batch of the scene queries (YCGE_CAMERA_HOST=1)
int tick_on_host(ycge_ctx *c, Tick &t)
{
    float rays[kMaxWindow * 8], hits[kMaxWindow * 10];
    int32_t ids[kMaxWindow * 2];
    return cam_run_host(t, [&](const Ray *r, int n, Hit *h) {
        for (int k = 0; k < n; k++) {
            float *q = rays + 8 * k;
            q[0] = r[k].o[0]; q[1] = r[k].o[1]; q[2] = r[k].o[2]; q[3] = r[k].d[0]; q[4] = r[k].d[1]; q[5] = r[k].d[2]; q[6] = r[k].tmin; q[7] = r[k].tmax;
        }
        const int e = query_hit_batch(c, "ycge_volume_camera_tick", rays, n, hits, ids);
        if (e != YCGE_OK) return e;
        for (int k = 0; k < n; k++) {
            h[k].hit = ids[2 * k] >= 0 ? 1 : 0;
            h[k].t = hits[10 * k]; h[k].nx = hits[10 * k + 4]; h[k].ny = hits[10 * k + 5]; h[k].nz = hits[10 * k + 6];
        }
        return 0;
    }, kMaxWindow);
}

// one launch, one read-back, one synchronise
int tick_on_device(ycge_ctx *c, Tick &t, const ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves, int32_t n_moves,
                   float dt_ms, int32_t run_update)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->query) c->query.reset(new QueryState());
    QueryState &Q = *c->query;
    HIP_TRY(c, Q.stream.ensure());
    HIP_TRY(c, Q.cam_spill.reserve((size_t)(c->spill_levels > 0 ? c->spill_levels : 1) * 64));
    HIP_TRY(c, Q.cam_dev.reserve(sizeof(TickIn) + sizeof(TickOut)));
    HIP_TRY(c, Q.cam_stage.reserve(sizeof(TickIn) + sizeof(TickOut)));
    TickIn *in = reinterpret_cast<TickIn *>(Q.cam_stage.data());
    TickOut *out = reinterpret_cast<TickOut *>(Q.cam_stage.data() + sizeof(TickIn));
    std::memset(in, 0, sizeof(TickIn));
    in->body = *body; in->world = *world; in->dt_ms = dt_ms; in->n_moves = n_moves; in->run_update = run_update;
    if (n_moves > 0) std::memcpy(in->moves, moves, sizeof(ycge_camera_move) * (size_t)n_moves);
    std::memset(out, 0xff, sizeof(TickOut));                                  // (no record is read as one unless the kernel stored it)
    uint8_t *d_in = Q.cam_dev.p, *d_out = Q.cam_dev.p + sizeof(TickIn);
    HIP_TRY(c, hipMemcpyAsync(d_in, in, sizeof(TickIn) + sizeof(TickOut), hipMemcpyHostToDevice, Q.stream));
    if (c->scene_ev) HIP_TRY(c, hipStreamWaitEvent(Q.stream, c->scene_ev, 0));
    const int e = ycge_launch_camera_tick(&c->sd, d_in, d_out, Q.cam_spill.p, c->has_grid ? 1 : 0, Q.stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "ycge_volume_camera_tick: k_camera_tick launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(out, d_out, sizeof(TickOut), hipMemcpyDeviceToHost, Q.stream));
    HIP_TRY(c, hipStreamSynchronize(Q.stream));
    if (out->status < ST_OK || out->status > ST_NOT_FINITE) return c->fail(YCGE_ERR_DEVICE, "ycge_volume_camera_tick: k_camera_tick stored no record");
    t.b = out->body; t.info = out->info; t.status = out->status; t.bad_move = out->bad_move;
    return YCGE_OK;
}

int camera_tick(ycge_ctx *c, ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves, int32_t n_moves, float dt_ms,
                int32_t run_update, ycge_camera_tick_info *info)
{
    const char *fn = "ycge_volume_camera_tick";
    char msg[256];
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    int32_t bad = -1;
    if (const char *why = cam_refusal(body, world, moves, n_moves, dt_ms, &bad)) {
        const int rc = refuse_text(msg, sizeof msg, fn, why, bad);
        return c->fail(rc, "%s", msg);
    }
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "Scene BVH not built; call ycge_scene_upload first (Scene.cs:73)");
    Tick t;
    const char *env = std::getenv("YCGE_CAMERA_HOST");
    if (env && env[0] == '1') {
        cam_begin(t, *body, kDefaultShape, *world, moves, n_moves, dt_ms, run_update);
        const int e = tick_on_host(c, t);
        if (e != YCGE_OK) return e;
    } else {
        t = Tick();
        const int e = tick_on_device(c, t, body, world, moves, n_moves, dt_ms, run_update);
        if (e != YCGE_OK) return e;
    }
    if (t.status != ST_OK) {
        const int rc = status_text(msg, sizeof msg, fn, t.status, t.bad_move);
        return c->fail(rc, "%s", msg);
    }
    *body = t.b;
    if (info) *info = t.info;
    return YCGE_OK;
}

} // namespace
} // namespace ycge_host

namespace ycge_host {
namespace {

// YCGE_CAMERA_HOST=1: a round collects the next window of every body still running into one batch of the scene queries, then commits
// body by body
int bodies_on_host(ycge_ctx *c, std::vector<Tick> &ticks)
{
    const size_t n = ticks.size();
    std::vector<float> rays, hits;
    std::vector<int32_t> ids, taken(n);
    for (;;) {
        rays.clear();
        for (size_t i = 0; i < n; i++) {
            Tick &t = ticks[i];
            taken[i] = 0;
            if (!cam_running(t)) continue;
            taken[i] = cam_take(t, kMaxWindow);
            for (int k = 0; k < taken[i]; k++) {
                Ray r;
                cam_ray(t, t.gi + k, r);
                const float q[8] = {r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], r.tmin, r.tmax};
                rays.insert(rays.end(), q, q + 8);
            }
        }
        const size_t total = rays.size() / 8;
        if (total == 0) return YCGE_OK;
        hits.resize(total * 10); ids.resize(total * 2);
        const int e = query_hit_batch(c, "ycge_volume_bodies_tick", rays.data(), (int32_t)total, hits.data(), ids.data());
        if (e != YCGE_OK) return e;
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            if (taken[i] == 0) continue;
            Hit h[kMaxWindow];
            for (int k = 0; k < taken[i]; k++, at++) {
                h[k].hit = ids[2 * at] >= 0 ? 1 : 0;
                h[k].t = hits[10 * at]; h[k].nx = hits[10 * at + 4]; h[k].ny = hits[10 * at + 5]; h[k].nz = hits[10 * at + 6];
            }
            cam_commit(ticks[i], h, taken[i]);
        }
    }
}

// one staged copy up, one launch of n workgroups, one copy back, one synchronise; the records back in `out` (n TickOut of the staging)
int bodies_on_device(ycge_ctx *c, const ycge_camera_body *bodies, const ycge_body_shape *shapes, int32_t n, const ycge_camera_world *world,
                     const ycge_camera_move *moves, const int32_t *move_first, float dt_ms, int32_t run_update, const TickOut **out_records)
{
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->query) c->query.reset(new QueryState());
    QueryState &Q = *c->query;
    HIP_TRY(c, Q.stream.ensure());
    const size_t total_moves = (size_t)move_first[n];
    const size_t off_in = sizeof(BodiesHeader), off_moves = off_in + sizeof(BodyIn) * (size_t)n;
    const size_t off_out = off_moves + sizeof(ycge_camera_move) * total_moves, bytes = off_out + sizeof(TickOut) * (size_t)n;
    // a column a lane of the whole grid (StackT::init: column blockIdx.x * 64 + threadIdx.x, stride 64 * n)
    HIP_TRY(c, Q.bodies_spill.reserve((size_t)(c->spill_levels > 0 ? c->spill_levels : 1) * 64 * (size_t)n));
    HIP_TRY(c, Q.bodies_dev.reserve(bytes));
    HIP_TRY(c, Q.bodies_stage.reserve(bytes));
    uint8_t *stage = Q.bodies_stage.data();
    BodiesHeader *hdr = reinterpret_cast<BodiesHeader *>(stage);
    BodyIn *in = reinterpret_cast<BodyIn *>(stage + off_in);
    TickOut *out = reinterpret_cast<TickOut *>(stage + off_out);
    std::memset(stage, 0, off_moves);
    hdr->world = *world; hdr->dt_ms = dt_ms; hdr->run_update = run_update; hdr->n = n; hdr->n_moves_total = (int32_t)total_moves;
    for (int32_t i = 0; i < n; i++) {
        in[i].body = bodies[i];
        in[i].shape = shapes ? shapes[i] : kDefaultShape;
        in[i].first_move = move_first[i]; in[i].n_moves = move_first[i + 1] - move_first[i];
    }
    if (total_moves > 0) std::memcpy(stage + off_moves, moves, sizeof(ycge_camera_move) * total_moves);
    std::memset(out, 0xff, sizeof(TickOut) * (size_t)n);                       // (no record is read as one unless the kernel stored it)
    uint8_t *dev = Q.bodies_dev.p;
    HIP_TRY(c, hipMemcpyAsync(dev, stage, bytes, hipMemcpyHostToDevice, Q.stream));
    if (c->scene_ev) HIP_TRY(c, hipStreamWaitEvent(Q.stream, c->scene_ev, 0));
    const int e = ycge_launch_bodies_tick(&c->sd, dev, dev + off_in, dev + off_moves, dev + off_out, Q.bodies_spill.p, n, c->has_grid ? 1 : 0, Q.stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "ycge_volume_bodies_tick: k_bodies_tick launch failed: %s", hipGetErrorString((hipError_t)e));
    HIP_TRY(c, hipMemcpyAsync(out, dev + off_out, sizeof(TickOut) * (size_t)n, hipMemcpyDeviceToHost, Q.stream));
    HIP_TRY(c, hipStreamSynchronize(Q.stream));
    for (int32_t i = 0; i < n; i++)
        if (out[i].status < ST_OK || out[i].status > ST_NOT_FINITE) return c->fail(YCGE_ERR_DEVICE, "ycge_volume_bodies_tick: k_bodies_tick stored no record for body %d", i);
    *out_records = out;
    return YCGE_OK;
}

int bodies_tick(ycge_ctx *c, ycge_camera_body *bodies, const ycge_body_shape *shapes, int32_t n, const ycge_camera_world *world,
                const ycge_camera_move *moves, const int32_t *move_first, float dt_ms, int32_t run_update, ycge_body_result *results,
                ycge_camera_tick_info *info)
{
    char msg[256];
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    const int rc = bodies_refusal(msg, sizeof msg, "ycge_volume_bodies_tick", bodies, shapes, n, world, moves, move_first, dt_ms, results);
    if (rc != YCGE_OK) return c->fail(rc, "%s", msg);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "Scene BVH not built; call ycge_scene_upload first (Scene.cs:73)");
    if (n == 0) return YCGE_OK;
    const char *env = std::getenv("YCGE_CAMERA_HOST");
    if (env && env[0] == '1') {
        std::vector<Tick> ticks((size_t)n);
        for (int32_t i = 0; i < n; i++) begin_body(ticks[(size_t)i], i, bodies, shapes, world, moves, move_first, dt_ms, run_update);
        const int e = bodies_on_host(c, ticks);
        if (e != YCGE_OK) return e;
        for (int32_t i = 0; i < n; i++) {
            const Tick &t = ticks[(size_t)i];
            commit_body(i, t.b, t.info, t.status, t.bad_move, bodies, results, info);
        }
        return YCGE_OK;
    }
    const TickOut *out = nullptr;
    const int e = bodies_on_device(c, bodies, shapes, n, world, moves, move_first, dt_ms, run_update, &out);
    if (e != YCGE_OK) return e;
    for (int32_t i = 0; i < n; i++) commit_body(i, out[i].body, out[i].info, out[i].status, out[i].bad_move, bodies, results, info);
    return YCGE_OK;
}

} // namespace
} // namespace ycge_host

extern "C" int ycge_volume_bodies_tick(ycge_ctx *c, ycge_camera_body *bodies, const ycge_body_shape *shapes, int32_t n, const ycge_camera_world *world,
                                       const ycge_camera_move *moves, const int32_t *move_first, float delta_time_ms, int32_t run_update,
                                       ycge_body_result *results, ycge_camera_tick_info *info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return ycge_host::bodies_tick(c, bodies, shapes, n, world, moves, move_first, delta_time_ms, run_update, results, info);
}
catch (...) { return ycge_host::abi_catch(c); }

extern "C" int ycge_volume_camera_tick(ycge_ctx *c, ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves,
                                       int32_t n_moves, float delta_time_ms, int32_t run_update, ycge_camera_tick_info *info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return ycge_host::camera_tick(c, body, world, moves, n_moves, delta_time_ms, run_update, info);
}
catch (...) { return ycge_host::abi_catch(c); }

#endif
