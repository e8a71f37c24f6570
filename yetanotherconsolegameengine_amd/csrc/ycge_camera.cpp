// ycge_camera.cpp - VolumeScene's camera physics as one call a tick (ycge_volume_camera_tick; kernel: ycge_camera.hip; the stepper both
// sides run: ycge_camera_physics.h).
//
// The device route stages {body, world, moves} up through page-locked memory, waits for the device work of the last scene change
// (scene_ev, as a query does), launches k_camera_tick - one wavefront that runs the whole chain of rays and its control - reads the
// kernel's one record back and synchronises the query stream: one launch, one read-back, one synchronise.  It runs on the query stream
// with buffers of its own, so it waits for no frame in flight and writes nothing a frame reads.  *body and *info are written from the
// record on success only.  YCGE_CAMERA_HOST=1 runs the same stepper here, each window one batch of the scene queries' own run.
//
// ycge_test_camera_tick_host (include/ycge_hooks.h) is the stepper over a caller's Scene.Hit: no context, no device.  With
// -DYCGE_CAMERA_HOOK_ONLY this file is that hook alone and needs no HIP (a stand-alone sanitizer build of the stepper).
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

} // namespace

extern "C" int ycge_test_camera_tick_host(ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves, int32_t n_moves,
                                          float delta_time_ms, int32_t run_update, ycge_camera_tick_info *info, ycge_camera_hit_fn hit, void *user,
                                          int32_t windowed, char *msg, size_t msg_bytes)
try {
    const char *fn = "ycge_test_camera_tick_host";
    int32_t bad = -1;
    if (const char *why = cam_refusal(body, world, moves, n_moves, delta_time_ms, &bad)) return refuse_text(msg, msg_bytes, fn, why, bad);
    if (!hit) return refuse_text(msg, msg_bytes, fn, "NULL hit callback", -1);
    Tick t;
    cam_begin(t, *body, *world, moves, n_moves, delta_time_ms, run_update);
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
        cam_begin(t, *body, *world, moves, n_moves, dt_ms, run_update);
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

extern "C" int ycge_volume_camera_tick(ycge_ctx *c, ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves,
                                       int32_t n_moves, float delta_time_ms, int32_t run_update, ycge_camera_tick_info *info)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return ycge_host::camera_tick(c, body, world, moves, n_moves, delta_time_ms, run_update, info);
}
catch (...) { return ycge_host::abi_catch(c); }

#endif
