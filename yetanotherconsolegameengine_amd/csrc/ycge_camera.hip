// ycge_camera.hip - the kernels of the camera tick (ycge_volume_camera_tick) and of many bodies a tick (ycge_volume_bodies_tick); host side:
// ycge_camera.cpp.
//
// Its own translation unit, as ycge_query.hip is: the walk is the frames' own (ycge_rt.hip.h: traverse, resolve_hit - included, not
// copied) and the code objects of ycge_kernels.hip stay exactly what they were.
#include <hip/hip_runtime.h>

#include "ycge_rt.hip.h"
#include "ycge_camera_physics.h"

namespace ycge {

// ---------------------------------------------------------------------------------- the camera tick (ycge_volume_camera_tick)
// One workgroup of one wavefront runs a whole tick of VolumeScene's camera physics: the stepper of ycge_camera_physics.h hands out
// windows of consecutive rays of the reference's serial order; lane k walks ray k of the window - Scene.Hit (Scene.cs:71-75) as
// k_query does it: traverse() from the scene root, resolve_hit() for the normal - and leaves {hit, t, n} in LDS; then EVERY lane folds
// the window in the reference's order (the control is uniform: 64 copies of the same state, no broadcast), which drops what lies behind
// a ray that changed the state.  The loop is bounded by the stepper's caps (YCGE_CAMERA_MAX_MOVES moves of at most
// YCGE_CAMERA_MAX_MICRO_STEPS micro-steps, a fixed number of groups an update, every window commits at least one ray).  Lane 0 stores
// the one result record with plain stores, the status last.

// the loop both kernels run: the tick `t` (begun by the caller) to its end, this wavefront's lanes the rays of each window
template <bool HAS_GRID>
__device__ __forceinline__ void run_tick(const SceneDev &S, ycge_cam::Tick &t, ycge_cam::Hit *s_hits, StackT<64> &st)
{
    Work w = {0, 0, 0, 0, 0, 0, 0};
    const int lane = (int)threadIdx.x;
    while (ycge_cam::cam_running(t)) {
        const int n = ycge_cam::cam_take(t, ycge_cam::kMaxWindow);
        if (lane < n) {
            ycge_cam::Ray r;
            ycge_cam::cam_ray(t, t.gi + lane, r);
            RayQ q;
            q.o = f3(r.o[0], r.o[1], r.o[2]);
            q.d = normalized(f3(r.d[0], r.d[1], r.d[2]));       // new Ray(o, d), Ray.cs:8-12
            q.tmin = r.tmin; q.tmax = r.tmax;
            q.anyhit = false;
            float tt = 0.0f;
            int prim = -1, sub = 0;
            traverse<false, HAS_GRID, false>(S, q, st, tt, prim, sub, w);
            ycge_cam::Hit h = {0, 0.0f, 0.0f, 0.0f, 0.0f};
            if (prim >= 0) {
                HitAttr a;
                resolve_hit<HAS_GRID>(S, prim, sub, tt, q.o, q.d, a);
                h.hit = 1; h.t = tt; h.nx = a.n.x; h.ny = a.n.y; h.nz = a.n.z;
            }
            s_hits[lane] = h;
        }
        __syncthreads();
        ycge_cam::cam_commit(t, s_hits, n);
        __syncthreads();
    }
}
// lane 0 stores the one record of a tick with plain stores, the status last
__device__ __forceinline__ void store_tick(const ycge_cam::Tick &t, ycge_cam::TickOut *out)
{
    if (threadIdx.x == 0) {
        out->body = t.b;
        out->info = t.info;
        out->bad_move = t.bad_move;
        out->status = t.status;
    }
}

template <bool HAS_GRID>
__global__ __launch_bounds__(64) void k_camera_tick(const SceneDev S, const ycge_cam::TickIn *in, ycge_cam::TickOut *out, void *spill)
{
    __shared__ ycge_cam::Hit s_hits[64];
    StackT<64> st;
    st.init(spill, 64);
    int32_t n_moves = in->n_moves;
    if (n_moves < 0) n_moves = 0;
    if (n_moves > YCGE_CAMERA_MAX_MOVES) n_moves = YCGE_CAMERA_MAX_MOVES;         // (the host refused these: never past the record)
    const ycge_body_shape shape = YCGE_BODY_SHAPE_DEFAULT;
    ycge_cam::Tick t;
    ycge_cam::cam_begin(t, in->body, shape, in->world, in->moves, n_moves, in->dt_ms, in->run_update);
    run_tick<HAS_GRID>(S, t, s_hits, st);
    store_tick(t, out);
}

// ---------------------------------------------------------------------------------- many bodies a tick (ycge_volume_bodies_tick)
// Workgroup b - one wavefront - runs body b's whole tick with k_camera_tick's loop, from its own input record, its own shape and its
// slice of the one shared array of moves, and stores its own result record.  The workgroups share nothing but the scene: a body's
// outcome is the serial stepper's on its inputs alone.  The spill area holds a column a lane of the WHOLE grid: lane l of workgroup b
// has column b * 64 + l (StackT::init) and strides by 64 * n, so the launch needs max(1, spill levels) * 64 * n entries.
template <bool HAS_GRID>
__global__ __launch_bounds__(64) void k_bodies_tick(const SceneDev S, const ycge_cam::BodiesHeader *hdr, const ycge_cam::BodyIn *in,
                                                    const ycge_camera_move *moves, ycge_cam::TickOut *out, void *spill)
{
    __shared__ ycge_cam::Hit s_hits[64];
    const uint32_t b = blockIdx.x;
    const int32_t n = hdr->n;
    if (n <= 0 || b >= (uint32_t)n || gridDim.x != (uint32_t)n) return;           // (the launch is n workgroups: the spill area is sized by it)
    StackT<64> st;
    st.init(spill, 64u * (uint32_t)n);
    const ycge_cam::BodyIn *rec = in + b;
    int32_t first = rec->first_move, n_moves = rec->n_moves;
    if (n_moves < 0) n_moves = 0;
    if (n_moves > YCGE_CAMERA_MAX_MOVES) n_moves = YCGE_CAMERA_MAX_MOVES;
    if (first < 0 || first > hdr->n_moves_total - n_moves) { first = 0; n_moves = 0; }      // (the host refused these: never past the array)
    ycge_cam::Tick t;
    ycge_cam::cam_begin(t, rec->body, rec->shape, hdr->world, moves + first, n_moves, hdr->dt_ms, hdr->run_update);
    run_tick<HAS_GRID>(S, t, s_hits, st);
    store_tick(t, out + b);
}

} // namespace ycge

extern "C" {

int ycge_launch_camera_tick(const ycge::SceneDev *S, const void *in, void *out, void *spill, int has_grid, hipStream_t stream)
{
    using namespace ycge;
    const dim3 grid(1), block(64);
    if (has_grid) hipLaunchKernelGGL((k_camera_tick<true>), grid, block, 0, stream, *S, (const ycge_cam::TickIn *)in, (ycge_cam::TickOut *)out, spill);
    else hipLaunchKernelGGL((k_camera_tick<false>), grid, block, 0, stream, *S, (const ycge_cam::TickIn *)in, (ycge_cam::TickOut *)out, spill);
    return (int)hipGetLastError();
}

int ycge_launch_bodies_tick(const ycge::SceneDev *S, const void *header, const void *in, const void *moves, void *out, void *spill, int n, int has_grid,
                            hipStream_t stream)
{
    using namespace ycge;
    if (n < 1 || n > YCGE_BODIES_MAX) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)n), block(64);
    if (has_grid) hipLaunchKernelGGL((k_bodies_tick<true>), grid, block, 0, stream, *S, (const ycge_cam::BodiesHeader *)header, (const ycge_cam::BodyIn *)in,
                                     (const ycge_camera_move *)moves, (ycge_cam::TickOut *)out, spill);
    else hipLaunchKernelGGL((k_bodies_tick<false>), grid, block, 0, stream, *S, (const ycge_cam::BodiesHeader *)header, (const ycge_cam::BodyIn *)in,
                            (const ycge_camera_move *)moves, (ycge_cam::TickOut *)out, spill);
    return (int)hipGetLastError();
}

} // extern "C"
