// ycge_query.cpp - Scene.Hit / Scene.Occluded as batched queries on the device scene (ycge_scene_hit, ycge_scene_occluded).
//
// The other caller of Scene.Hit in the reference - VolumeScene's camera physics (ground fan, collision capsule, push-out) - asks a few
// rays per Update, between two frames, and may do so while a frame is in flight.  So a query runs on a stream of its own with buffers of
// its own: it waits for the device work of the last scene change (scene_ev on the context's stream) and for nothing a frame queued after
// it, and it writes nothing a frame reads.  The call returns with the results in the caller's arrays (page-locked staging both ways, as
// ycge_scene_update_texture does; the caller's arrays are its own again on return).  Scene changes quiesce the device first, so the scene
// buffers are read-only while a query runs.
#include "ycge_ctx.h"

namespace ycge_host {

int query_scene_changed(ycge_ctx *c)
{
    HIP_TRY(c, c->scene_ev.ensure());
    HIP_TRY(c, hipEventRecord(c->scene_ev, c->stream));
    return YCGE_OK;
}

namespace {

// why ray i was refused (the device reported its index; the reason is recomputed here for that one ray)
int refuse_ray(ycge_ctx *c, const char *fn, const float *rays, uint32_t i)
{
    const float *r = rays + (size_t)i * 8;
    const char *why = "direction is not normalisable (dx*dx + dy*dy + dz*dz is not a finite positive binary32)";
    for (int k = 0; k < 3; k++) if (!std::isfinite(r[k])) why = "origin is not finite";
    if (std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2])) {
        if (!std::isfinite(r[3]) || !std::isfinite(r[4]) || !std::isfinite(r[5])) why = "direction is not finite";
        else if (!std::isfinite(r[6])) why = "tmin is not finite";
        else if (std::isnan(r[7])) why = "tmax is NaN";
    }
    return c->fail(YCGE_ERR_INVALID_ARG, "%s: ray %u: %s", fn, i, why);
}

// one batch: hits / ids (closest hit) or occluded (the boolean)
int run_query(ycge_ctx *c, const char *fn, const float *rays, int32_t n, float *hits, int32_t *ids, uint8_t *occluded)
{
    if (c->parent) return c->fail(YCGE_ERR_INVALID_ARG, "peer contexts are driven by their root");
    if (n < 0) return c->fail(YCGE_ERR_INVALID_ARG, "%s: n = %d", fn, n);
    if (n > 0 && (!rays || (occluded ? false : (!hits || !ids)))) return c->fail(YCGE_ERR_INVALID_ARG, "%s: null array with n = %d", fn, n);
    if (!c->have_scene) return c->fail(YCGE_ERR_NO_SCENE, "Scene BVH not built; call ycge_scene_upload first (Scene.cs:73)");
    if (n == 0) return YCGE_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->query) c->query.reset(new QueryState());
    QueryState &Q = *c->query;
    HIP_TRY(c, Q.stream.ensure());
    const int has_grid = c->has_grid ? 1 : 0, occl = occluded ? 1 : 0;
    uint32_t &lanes = Q.lanes[has_grid * 2 + occl];
    if (!lanes) lanes = ycge_launch_query_lanes(has_grid, occl, c->compute_units);
    const size_t un = (size_t)n;
    HIP_TRY(c, Q.spill.reserve((size_t)(c->spill_levels > 0 ? c->spill_levels : 1) * lanes));
    HIP_TRY(c, Q.rays.reserve(8 * un));
    HIP_TRY(c, Q.first_bad.reserve(1));
    if (occl) HIP_TRY(c, Q.occluded.reserve(un));
    else { HIP_TRY(c, Q.hits.reserve(10 * un)); HIP_TRY(c, Q.ids.reserve(2 * un)); }
    const size_t in_bytes = 32 * un, out_bytes = 64 + (occl ? un : 48 * un);       // out: {first bad ray, pad} then the records
    HIP_TRY(c, Q.in_stage.reserve(in_bytes)); HIP_TRY(c, Q.out_stage.reserve(out_bytes));
    std::memcpy(Q.in_stage.p, rays, in_bytes);
    HIP_TRY(c, hipMemcpyAsync(Q.rays.p, Q.in_stage.p, in_bytes, hipMemcpyHostToDevice, Q.stream));
    if (c->scene_ev) HIP_TRY(c, hipStreamWaitEvent(Q.stream, c->scene_ev, 0));
    HIP_TRY(c, hipMemsetAsync(Q.first_bad.p, 0xff, sizeof(uint32_t), Q.stream));
    const int e = ycge_launch_query(&c->sd, Q.rays.p, (uint32_t)n, Q.hits.p, Q.ids.p, occl ? Q.occluded.p : nullptr, Q.first_bad.p, Q.spill.p, lanes, has_grid, Q.stream);
    if (e != 0) return c->fail(YCGE_ERR_DEVICE, "%s: k_query launch failed: %s", fn, hipGetErrorString((hipError_t)e));
    uint8_t *out = Q.out_stage.data();
    HIP_TRY(c, hipMemcpyAsync(out, Q.first_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, Q.stream));
    if (occl) HIP_TRY(c, hipMemcpyAsync(out + 64, Q.occluded.p, un, hipMemcpyDeviceToHost, Q.stream));
    else {
        HIP_TRY(c, hipMemcpyAsync(out + 64, Q.hits.p, 40 * un, hipMemcpyDeviceToHost, Q.stream));
        HIP_TRY(c, hipMemcpyAsync(out + 64 + 40 * un, Q.ids.p, 8 * un, hipMemcpyDeviceToHost, Q.stream));
    }
    HIP_TRY(c, hipStreamSynchronize(Q.stream));
    uint32_t bad;
    std::memcpy(&bad, out, sizeof bad);
    if (bad != UINT32_MAX) return refuse_ray(c, fn, rays, bad);
    if (occl) std::memcpy(occluded, out + 64, un);
    else { std::memcpy(hits, out + 64, 40 * un); std::memcpy(ids, out + 64 + 40 * un, 8 * un); }
    return YCGE_OK;
}

} // namespace

int query_hit_batch(ycge_ctx *c, const char *fn, const float *rays, int32_t n, float *hits, int32_t *ids) { return run_query(c, fn, rays, n, hits, ids, nullptr); }

} // namespace ycge_host

// =========================================================================== C-ABI
extern "C" {

int ycge_scene_hit(ycge_ctx *c, const float *rays, int32_t n, float *hits, int32_t *ids)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    return run_query(c, "ycge_scene_hit", rays, n, hits, ids, nullptr);
}
catch (...) { return ycge_host::abi_catch(c); }

int ycge_scene_occluded(ycge_ctx *c, const float *rays, int32_t n, uint8_t *occluded)
try {
    if (!c) return YCGE_ERR_INVALID_ARG;
    if (n > 0 && !occluded) return c->fail(YCGE_ERR_INVALID_ARG, "ycge_scene_occluded: null array with n = %d", n);
    return run_query(c, "ycge_scene_occluded", rays, n, nullptr, nullptr, occluded);
}
catch (...) { return ycge_host::abi_catch(c); }

} // extern "C"
