// ycge_camera_physics.h - VolumeScene's camera physics (Scenes/VolumeScenes.cs:51-159 Update, :165-213 HandleInput's effect on the body,
// :219-530 the helpers) as ONE stepper for host and device: a state machine over windows of rays.  Arithmetic and control only - who
// answers Scene.Hit is the caller's business (k_camera_tick: one lane a ray; the host: a batch of ycge_scene_hit or a test's callback).
//
// The serial order of the reference is a chain of Scene.Hit calls.  The stepper cuts it into GROUPS - the capsule's 6 rays of a
// micro-step, one vertical ray, the embed test's 8, the exit search's 12, a push-out call's 32 (2 passes x 8 directions x 2 heights), a
// ground fan's 5 - and hands out WINDOWS: the next rays of the current group as they are if no earlier ray of the window changes the
// state.  cam_commit folds a window's results in the reference's order and stops behind the first ray that did change it (best /
// blockNormal of the capsule, CameraPos of the push-out); the rest of the window is discarded and asked again from the new state.
// Scene.Hit is a pure function of its ray, so the committed results are those of the serial order, bit for bit, whatever the window
// size; a window of one ray IS the serial order.
//
// Types are the reference's: CameraPos is three binary32 (Vec3), `new Vec3(double, double, double)` rounds each component, the locals
// are double where the C# declares double, float where the operands are float (CameraPos.Y + StepUpGuardEpsilon is a binary32 sum).
// Compiled with -ffp-contract=off like everything else.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ycge.h"
#include "ycge_math.h"

namespace ycge_cam {

// VolumeScenes.cs:20-39.  EyeHeight, CollisionRadius, ProbeRadius, GroundClearance, JumpSpeed and GravityAccel are a body's shape
// (ycge_body_shape, Tick::s): data, read in the types and the order of operations the reference uses its constants in - widened where
// the C# widens a const float, so a shape of the reference's values gives the reference's bits.
constexpr float kMaxProbeHeight = 4096.0f;
constexpr float kLocalProbeDepthMin = 3.0f, kLocalProbeStart = 0.6f, kExtraFallMargin = 1.0f, kStepUpGuardEpsilon = 0.05f;
constexpr float kShiftHoldGraceSeconds = 0.15f;

struct Ray { float o[3], d[3], tmin, tmax; };      // d as it is handed to `new Ray(o, d)`: whoever walks it normalises (Ray.cs:8-12)
struct Hit { int32_t hit; float t, nx, ny, nz; };  // the boolean of Scene.Hit, rec.T, rec.N

enum { G_NONE = 0, G_CAPS, G_VERT, G_EMBED, G_EXIT, G_PUSH, G_FAN };
enum { PC_MOVE_NEXT = 0, PC_H_HEAD, PC_H_END, PC_V_HEAD, PC_V_END, PC_UPDATE, PC_EMBED_END, PC_EXIT_END, PC_PUSH2, PC_AFTER_RESOLVE, PC_AUTO_END,
       PC_GROUND_END, PC_CORR_END, PC_FINAL_PUSH, PC_FAILSAFE, PC_DONE };
enum { ST_OK = 0, ST_CAP_HORIZONTAL = 1, ST_CAP_VERTICAL = 2, ST_NOT_FINITE = 3 };
constexpr int kMaxWindow = 32;     // the largest group (a push-out call)

struct Tick {
    ycge_camera_body b;
    ycge_body_shape s;
    ycge_camera_world w;
    const ycge_camera_move *moves;
    int32_t n_moves, run_update;
    float dt_ms;
    ycge_camera_tick_info info;
    int32_t status, bad_move;     // ST_*; the move a cap was reached in
    int32_t pc, grp, gi, gn, mv;
    float dts;                    // Update's dt in seconds
    // AttemptMoveHorizontal / AttemptMoveVertical
    double remaining, step, best, vsign;
    float dirx, dirz, perpx, perpz, bnx, bny, bnz, vt;
    int32_t had, micro, vhit;
    // eye / torso heights of the running helper
    double ey, ty;
    // ResolveIfEmbedded
    float probe, search_r;
    int32_t ebits, found, best_dir;
    double best_t;
    // TrySampleGroundYFan
    double fx, fz, fstart, fmax, best_ok, ground, new_y;
    int32_t any_hit, any_ok, fan_has;
};

// Math.Max / Math.Min on doubles (NaN wins, +0 > -0)
YCGE_HD double dmax(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a == b) return signbit(a) ? b : a;
    return a > b ? a : b;
}
YCGE_HD double dmin(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    if (a == b) return signbit(a) ? a : b;
    return a < b ? a : b;
}
YCGE_HD bool finite3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

YCGE_HD void set_group(Tick &t, int grp, int n, int next_pc) { t.grp = grp; t.gi = 0; t.gn = n; t.pc = next_pc; }
YCGE_HD void heights(Tick &t)          // double eyeY = CameraPos.Y; double torsoY = CameraPos.Y - (EyeHeight * 0.5);
{
    t.ey = (double)t.b.pos[1];
    t.ty = (double)t.b.pos[1] - ((double)t.s.eye_height * 0.5);
}
YCGE_HD void start_push(Tick &t, int next_pc) { heights(t); set_group(t, G_PUSH, 32, next_pc); }     // ApplyWallRepulsion, :418-440
YCGE_HD void start_fan(Tick &t, double x, double z, double start_y, double max_distance, int next_pc)   // TrySampleGroundYFan, :478-492
{
    t.fx = x; t.fz = z; t.fstart = start_y; t.fmax = max_distance;
    t.any_hit = 0; t.any_ok = 0; t.fan_has = 0;
    t.best_ok = -(double)YCGE_INF; t.ground = -(double)YCGE_INF;
    set_group(t, G_FAN, 5, next_pc);
}
YCGE_HD void fail(Tick &t, int status) { t.status = status; t.bad_move = t.mv - 1; t.grp = G_NONE; t.pc = PC_DONE; }

// runs the control between two groups of rays: returns with a group set up (t.grp != G_NONE) or with the tick over (t.pc == PC_DONE)
YCGE_HD void cam_control(Tick &t)
{
    float *pos = t.b.pos;
    while (t.grp == G_NONE && t.pc != PC_DONE) {
        if (!finite3(pos)) { fail(t, ST_NOT_FINITE); return; }
        switch (t.pc) {
        case PC_MOVE_NEXT: {
            if (t.mv >= t.n_moves) { t.pc = PC_UPDATE; break; }
            const ycge_camera_move m = t.moves[t.mv++];
            if (m.kind == YCGE_CAMERA_MOVE_SHIFT) {
                t.b.shift_hold_timer = kShiftHoldGraceSeconds;                                      // :177
            } else if (m.kind == YCGE_CAMERA_MOVE_JUMP) {
                if (!m.shift && t.b.is_grounded) { t.b.vertical_velocity = t.s.jump_speed; t.b.is_grounded = 0; }    // :208-212
            } else if (m.kind == YCGE_CAMERA_MOVE_HORIZONTAL) {                                   // AttemptMoveHorizontal(delta), :219-227
                const float dx = m.a, dz = m.b;
                t.remaining = sqrt((double)(dx * dx + dz * dz));
                if (t.remaining <= 1e-6) break;
                t.dirx = (float)((double)dx / t.remaining); t.dirz = (float)((double)dz / t.remaining);
                t.perpx = -t.dirz; t.perpz = t.dirx;
                t.micro = 0;
                t.pc = PC_H_HEAD;
            } else {                                                                              // AttemptMoveVertical(dy), :300-305
                const double dy = (double)m.a;
                if (fabs(dy) <= 1e-6) break;
                t.remaining = fabs(dy);
                t.vsign = dy > 0.0 ? 1.0 : -1.0;
                t.micro = 0;
                t.pc = PC_V_HEAD;
            }
            break;
        }
        case PC_H_HEAD: {                                                                         // :228-241
            if (!(t.remaining > 1e-6)) { t.pc = PC_MOVE_NEXT; break; }
            if (t.micro >= YCGE_CAMERA_MAX_MICRO_STEPS) { fail(t, ST_CAP_HORIZONTAL); return; }
            t.micro++; t.info.micro_steps++;
            t.step = dmin(t.remaining, dmax(0.1, (double)t.s.collision_radius * 0.35));
            t.best = t.step; t.had = 0; t.bnx = t.bny = t.bnz = 0.0f;
            heights(t);
            set_group(t, G_CAPS, 6, PC_H_END);
            break;
        }
        case PC_H_END: {                                                                          // :254-277
            if (t.best <= 1e-5) { t.info.blocked_steps++; t.pc = PC_MOVE_NEXT; break; }
            pos[0] = (float)((double)pos[0] + (double)t.dirx * t.best);
            pos[2] = (float)((double)pos[2] + (double)t.dirz * t.best);
            t.remaining -= t.best;
            const double residual = t.step - t.best;
            if (residual > 1e-6 && t.had) {
                // ProjectOntoPlaneXZ(dir, blockNormal), :466-474
                float sx = 0.0f, sz = 0.0f;
                const float nl = ycge::cs_sqrt(t.bnx * t.bnx + t.bnz * t.bnz);
                if (!(nl <= 1e-6f)) {
                    const float nx = t.bnx / nl, nz = t.bnz / nl;
                    const float dot = t.dirx * nx + t.dirz * nz;
                    sx = t.dirx - dot * nx; sz = t.dirz - dot * nz;
                }
                const float len = ycge::cs_sqrt(sx * sx + sz * sz);
                if (len > 1e-6f) {
                    t.dirx = sx / len; t.dirz = sz / len;
                    t.remaining += residual;
                    t.info.slides++;
                }
            }
            t.pc = PC_H_HEAD;
            break;
        }
        case PC_V_HEAD: {                                                                         // :306-312
            if (!(t.remaining > 1e-6)) { t.pc = PC_MOVE_NEXT; break; }
            if (t.micro >= YCGE_CAMERA_MAX_MICRO_STEPS) { fail(t, ST_CAP_VERTICAL); return; }
            t.micro++; t.info.micro_steps++;
            t.step = dmin(t.remaining, dmax(0.1, (double)t.s.eye_height * 0.25));
            t.vhit = 0; t.vt = 0.0f;
            set_group(t, G_VERT, 1, PC_V_END);
            break;
        }
        case PC_V_END: {                                                                          // :313-323
            if (t.vhit) {
                const double cand = dmax(0.0, (double)t.vt - 0.01);
                if (cand <= 1e-5) { t.info.blocked_steps++; t.pc = PC_MOVE_NEXT; break; }
                pos[1] = (float)((double)pos[1] + cand * t.vsign);
            } else {
                pos[1] = (float)((double)pos[1] + t.step * t.vsign);
            }
            t.remaining -= t.step;
            t.pc = PC_V_HEAD;
            break;
        }
        case PC_UPDATE: {                                                                         // Update, :59-61, :72; IsLikelyEmbedded, :382-398
            if (!t.run_update) { t.pc = PC_DONE; break; }
            float dt = t.dt_ms;
            if (dt < 0.0f) dt = 0.0f;
            dt *= 0.001f;
            t.dts = dt;
            heights(t);
            t.probe = (float)dmax(0.05, (double)t.s.collision_radius * 0.25);
            t.ebits = 0;
            set_group(t, G_EMBED, 8, PC_EMBED_END);
            break;
        }
        case PC_EMBED_END: {                                                                      // ResolveIfEmbedded, :330-346
            if (!((t.ebits & 15) == 15 || (t.ebits >> 4) == 15)) { t.pc = PC_AFTER_RESOLVE; break; }
            heights(t);
            t.search_r = (float)dmax((double)t.s.collision_radius * 4.0, (double)t.w.voxel_size_y * 4.0);
            t.found = 0; t.best_t = (double)YCGE_INF; t.best_dir = 4;
            set_group(t, G_EXIT, 12, PC_EXIT_END);
            break;
        }
        case PC_EXIT_END: {                                                                       // :369-379
            if (t.found && t.best_t < (double)YCGE_INF) {
                const float dirs[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 0, 1}, {0, 0, -1}, {0, 1, 0}, {0, -1, 0}};
                const double eps = dmax(0.02, (double)t.w.voxel_size_y * 0.02);
                const float *d = dirs[t.best_dir];
                pos[0] = (float)((double)pos[0] + (double)d[0] * (t.best_t + eps));
                pos[1] = (float)((double)pos[1] + (double)d[1] * (t.best_t + eps));
                pos[2] = (float)((double)pos[2] + (double)d[2] * (t.best_t + eps));
                t.info.embedded_resolutions++;
                start_push(t, PC_PUSH2);
            } else {
                t.pc = PC_AFTER_RESOLVE;
            }
            break;
        }
        case PC_PUSH2:
            start_push(t, PC_AFTER_RESOLVE);
            break;
        case PC_AFTER_RESOLVE: {                                                                  // :75-106, :143-147
            if (!t.b.auto_placed) {
                const double probe_top = (double)ycge::cs_min(t.w.world_height + 16.0f, kMaxProbeHeight);
                start_fan(t, (double)pos[0], (double)pos[2], probe_top, probe_top + (double)8.0f, PC_AUTO_END);
                break;
            }
            if (t.b.shift_hold_timer > 0.0f) t.b.shift_hold_timer = ycge::cs_max(0.0f, t.b.shift_hold_timer - t.dts);
            if (!(t.b.shift_hold_timer > 0.0f)) {
                t.b.vertical_velocity -= t.s.gravity_accel * t.dts;
                t.new_y = (double)(pos[1] + t.b.vertical_velocity * t.dts);
                const double fall = dmax(0.0, (double)pos[1] - t.new_y);
                const double depth = dmax((double)kLocalProbeDepthMin, fall + (double)kExtraFallMargin);
                start_fan(t, (double)pos[0], (double)pos[2], (double)(pos[1] + kLocalProbeStart), depth + (double)kLocalProbeStart, PC_GROUND_END);
            } else {
                t.b.vertical_velocity = 0.0f;
                t.pc = PC_FINAL_PUSH;
            }
            break;
        }
        case PC_AUTO_END: {                                                                       // :78-85 (the early return)
            if (t.fan_has) pos[1] = (float)(t.ground + (double)t.s.eye_height + (double)t.s.ground_clearance);
            else pos[1] = t.w.water_level + t.s.eye_height + 4.0f;
            t.b.vertical_velocity = 0.0f;
            t.b.auto_placed = 1;
            t.info.auto_placements++;
            t.pc = PC_DONE;
            break;
        }
        case PC_GROUND_END: {                                                                     // :108-132
            t.b.is_grounded = 0;
            if (t.fan_has) {
                const double floor_y = t.ground + (double)t.s.eye_height + (double)t.s.ground_clearance;
                const bool above = floor_y > (double)(pos[1] + kStepUpGuardEpsilon);
                if (t.new_y <= floor_y && !above) {
                    t.new_y = floor_y;
                    t.b.vertical_velocity = 0.0f;
                    t.b.is_grounded = 1;
                    t.info.ground_snaps++;
                } else {
                    t.b.is_grounded = (!above && ((double)pos[1] - floor_y) <= (double)kStepUpGuardEpsilon) ? 1 : 0;
                }
            }
            pos[1] = (float)t.new_y;
            start_fan(t, (double)pos[0], (double)pos[2], (double)(pos[1] + kLocalProbeStart), (double)kLocalProbeStart + 1.5, PC_CORR_END);
            break;
        }
        case PC_CORR_END: {                                                                       // :132-141
            if (t.fan_has) {
                const double f2 = t.ground + (double)t.s.eye_height + (double)t.s.ground_clearance;
                if (f2 <= (double)(pos[1] + kStepUpGuardEpsilon) && ((double)pos[1] - f2) <= 0.5) {
                    pos[1] = (float)f2;
                    t.b.vertical_velocity = 0.0f;
                    t.b.is_grounded = 1;
                    t.info.ground_snaps++;
                }
            }
            t.pc = PC_FINAL_PUSH;
            break;
        }
        case PC_FINAL_PUSH:                                                                       // :150
            start_push(t, PC_FAILSAFE);
            break;
        case PC_FAILSAFE: {                                                                       // :153-158
            if ((double)pos[1] < -10.0) {
                pos[1] = 200.0f;
                t.b.vertical_velocity = 0.0f;
                t.b.repel_vel[0] = t.b.repel_vel[1] = t.b.repel_vel[2] = 0.0f;
                t.info.fail_safes++;
            }
            t.pc = PC_DONE;
            break;
        }
        default:
            t.pc = PC_DONE;
            break;
        }
    }
    if (t.pc == PC_DONE && t.status == ST_OK && !finite3(pos)) fail(t, ST_NOT_FINITE);
}

YCGE_HD void cam_begin(Tick &t, const ycge_camera_body &body, const ycge_body_shape &shape, const ycge_camera_world &world, const ycge_camera_move *moves,
                       int32_t n_moves, float dt_ms, int32_t run_update)
{
    t = Tick();
    t.b = body; t.s = shape; t.w = world; t.moves = moves; t.n_moves = n_moves; t.dt_ms = dt_ms; t.run_update = run_update;
    t.pc = PC_MOVE_NEXT; t.grp = G_NONE; t.bad_move = -1;
    cam_control(t);
}
YCGE_HD bool cam_running(const Tick &t) { return t.grp != G_NONE; }

// the next window: how many rays of the current group are asked now (at most max_rays; 1 = the serial order)
YCGE_HD int cam_take(Tick &t, int max_rays)
{
    int n = t.gn - t.gi;
    if (n > max_rays) n = max_rays;
    t.info.windows++;
    t.info.rays_walked += (uint32_t)n;
    return n;
}

// ray k (gi <= k < gn) of the current group, from the state as it is now
YCGE_HD void cam_ray(const Tick &t, int k, Ray &r)
{
    const float *pos = t.b.pos;
    switch (t.grp) {
    case G_CAPS: {                                   // :243-252: offsets {0, r, -r}, eye then torso; LimitStepByRay, :283-288
        const double offs[3] = {0.0, (double)t.s.collision_radius, -(double)t.s.collision_radius};
        const double o = offs[k >> 1];
        const float ox = (float)((double)t.perpx * o), oz = (float)((double)t.perpz * o);
        r.o[0] = pos[0] + ox; r.o[1] = (float)((k & 1) ? t.ty : t.ey); r.o[2] = pos[2] + oz;
        r.d[0] = t.dirx; r.d[1] = 0.0f; r.d[2] = t.dirz;
        r.tmin = 0.001f; r.tmax = (float)(t.best + 1e-3);
        break;
    }
    case G_VERT:                                     // :309-313
        r.o[0] = pos[0]; r.o[1] = pos[1]; r.o[2] = pos[2];
        r.d[0] = 0.0f; r.d[1] = (float)t.vsign; r.d[2] = 0.0f;
        r.tmin = 0.001f; r.tmax = (float)(t.step + 1e-3);
        break;
    case G_EMBED: {                                  // IsLikelyEmbeddedAtY, :389-405: +x, -x, +z, -z at the eye, then at the torso
        const int d = k & 3;
        r.o[0] = pos[0]; r.o[1] = (float)((k >> 2) ? t.ty : t.ey); r.o[2] = pos[2];
        r.d[0] = d == 0 ? 1.0f : d == 1 ? -1.0f : 0.0f; r.d[1] = 0.0f; r.d[2] = d == 2 ? 1.0f : d == 3 ? -1.0f : 0.0f;
        r.tmin = 0.0f; r.tmax = t.probe;
        break;
    }
    case G_EXIT: {                                   // :348-367: six axes, eye then torso
        const int d = k >> 1;
        r.o[0] = pos[0]; r.o[1] = (float)((k & 1) ? t.ty : t.ey); r.o[2] = pos[2];
        r.d[0] = d == 0 ? 1.0f : d == 1 ? -1.0f : 0.0f; r.d[1] = d == 4 ? 1.0f : d == 5 ? -1.0f : 0.0f; r.d[2] = d == 2 ? 1.0f : d == 3 ? -1.0f : 0.0f;
        r.tmin = 0.0f; r.tmax = t.search_r;
        break;
    }
    case G_PUSH: {                                   // :421-438, ResolvePenetrationAt :444-446
        const int d = (k >> 1) & 7;
        const double dx = (d == 0 || d == 4 || d == 5) ? 1.0 : (d == 1 || d == 6 || d == 7) ? -1.0 : 0.0;
        const double dz = (d == 2 || d == 4 || d == 6) ? 1.0 : (d == 3 || d == 5 || d == 7) ? -1.0 : 0.0;
        const double len = d < 4 ? 1.0 : 1.4142135623730951;      // Math.Sqrt(dx * dx + dz * dz)
        r.o[0] = pos[0]; r.o[1] = (float)((k & 1) ? t.ty : t.ey); r.o[2] = pos[2];
        r.d[0] = (float)(dx / len); r.d[1] = 0.0f; r.d[2] = (float)(dz / len);
        r.tmin = 0.001f; r.tmax = t.s.collision_radius;
        break;
    }
    default: {                                       // G_FAN: TrySampleGroundY, :520-525
        const double ox = k == 1 ? (double)t.s.probe_radius : k == 2 ? -(double)t.s.probe_radius : 0.0;
        const double oz = k == 3 ? (double)t.s.probe_radius : k == 4 ? -(double)t.s.probe_radius : 0.0;
        r.o[0] = (float)(t.fx + ox); r.o[1] = (float)t.fstart; r.o[2] = (float)(t.fz + oz);
        r.d[0] = 0.0f; r.d[1] = -1.0f; r.d[2] = 0.0f;
        r.tmin = 0.00001f; r.tmax = (float)t.fmax;
        break;
    }
    }
}

// folds the results of the window's rays gi .. gi + n - 1 in the reference's order; behind a ray that changed what the later rays of
// the window were made from, the rest is dropped.  When the group is over, the control runs on to the next group or to the end.
YCGE_HD void cam_commit(Tick &t, const Hit *hits, int n)
{
    float *pos = t.b.pos;
    for (int i = 0; i < n && t.gi < t.gn; i++) {
        const Hit h = hits[i];
        const int k = t.gi++;
        t.info.rays_committed++;
        bool changed = false;
        switch (t.grp) {
        case G_CAPS:                                 // LimitStepByRay, :288-297
            if (h.hit) {
                const double cand = dmax(0.0, (double)h.t - 0.01);
                if (cand < t.best) { t.best = cand; t.had = 1; t.bnx = h.nx; t.bny = h.ny; t.bnz = h.nz; changed = true; }
            }
            break;
        case G_VERT:
            t.vhit = h.hit ? 1 : 0; t.vt = h.t;
            break;
        case G_EMBED:                                // :386: the torso is asked only when the eye is not embedded
            if (h.hit) t.ebits |= 1 << k;
            if (k == 3 && (t.ebits & 15) == 15) t.gi = t.gn;
            break;
        case G_EXIT:                                 // :352-366
            if (h.hit && (double)h.t < t.best_t) { t.best_t = (double)h.t; t.best_dir = k >> 1; t.found = 1; }
            break;
        case G_PUSH:                                 // ResolvePenetrationAt, :446-463
            if (h.hit) {
                const float pen = t.s.collision_radius - h.t;
                if (pen > 0.0f) {
                    const float nl = ycge::cs_sqrt(h.nx * h.nx + h.nz * h.nz);
                    if (nl > 1e-6f) {
                        const float nx = h.nx / nl, nz = h.nz / nl;
                        const float push = pen + 0.01f;
                        pos[0] = pos[0] + nx * push;
                        pos[2] = pos[2] + nz * push;
                        t.info.push_outs++;
                        changed = true;
                    }
                }
            }
            break;
        default:                                     // G_FAN: :494-509, groundY = r.At(rec.T).Y
            if (h.hit) {
                const double y = (double)((float)t.fstart + -1.0f * h.t);
                t.any_hit = 1;
                const double floor_candidate = y + (double)t.s.eye_height + (double)t.s.ground_clearance;
                if (floor_candidate <= (double)(pos[1] + kStepUpGuardEpsilon)) {
                    if (!t.any_ok || y > t.best_ok) t.best_ok = y;
                    t.any_ok = 1;
                }
                if (!t.any_ok && (t.ground == -(double)YCGE_INF || y > t.ground)) t.ground = y;
            }
            break;
        }
        if (changed) break;
    }
    if (t.gi >= t.gn) {
        if (t.grp == G_FAN) {                        // :511-517
            if (t.any_ok) { t.ground = t.best_ok; t.fan_has = 1; }
            else t.fan_has = (t.any_hit && !(t.ground == -(double)YCGE_INF)) ? 1 : 0;
        }
        t.grp = G_NONE;
        cam_control(t);
    }
}

// what the exports refuse before any work: 0, or the reason (index of the move in *bad_move, -1: not a move)
YCGE_HD const char *cam_refusal(const ycge_camera_body *body, const ycge_camera_world *world, const ycge_camera_move *moves, int32_t n_moves,
                                float dt_ms, int32_t *bad_move)
{
    *bad_move = -1;
    if (!body || !world) return "NULL body or world";
    if (n_moves < 0 || n_moves > YCGE_CAMERA_MAX_MOVES) return "n_moves outside 0..YCGE_CAMERA_MAX_MOVES (32)";
    if (n_moves > 0 && !moves) return "NULL moves with n_moves > 0";
    if (!finite3(body->pos) || !isfinite(body->vertical_velocity) || !isfinite(body->shift_hold_timer) || !finite3(body->repel_vel))
        return "a field of the body is not finite";
    if (!isfinite(world->world_height) || !isfinite(world->water_level) || !isfinite(world->voxel_size_y)) return "a field of the world is not finite";
    if (!isfinite(dt_ms)) return "delta_time_ms is not finite";
    for (int32_t i = 0; i < n_moves; i++) {
        const ycge_camera_move &m = moves[i];
        *bad_move = i;
        if (m.kind < YCGE_CAMERA_MOVE_HORIZONTAL || m.kind > YCGE_CAMERA_MOVE_SHIFT) return "unknown kind";
        if (!isfinite(m.a) || !isfinite(m.b)) return "a field is not finite";
        if (m.kind == YCGE_CAMERA_MOVE_HORIZONTAL && !(sqrt((double)m.a * m.a + (double)m.b * m.b) <= (double)YCGE_CAMERA_MAX_MOVE_LENGTH))
            return "longer than YCGE_CAMERA_MAX_MOVE_LENGTH (64)";
        if (m.kind == YCGE_CAMERA_MOVE_VERTICAL && !(fabs((double)m.a) <= (double)YCGE_CAMERA_MAX_MOVE_LENGTH)) return "longer than YCGE_CAMERA_MAX_MOVE_LENGTH (64)";
    }
    *bad_move = -1;
    return nullptr;
}
// a shape the exports refuse: 0, or the reason.  The sizes are bounded like a move's length, so that a probe (4 radii in the exit
// search) and a push-out stay within the lengths YCGE_CAMERA_MAX_MOVE_LENGTH and the micro-step cap were set for
YCGE_HD const char *cam_shape_refusal(const ycge_body_shape &s)
{
    if (!isfinite(s.eye_height) || !isfinite(s.collision_radius) || !isfinite(s.probe_radius) || !isfinite(s.ground_clearance) || !isfinite(s.jump_speed) ||
        !isfinite(s.gravity_accel))
        return "a field of the shape is not finite";
    if (!(s.eye_height > 0.0f) || !(s.collision_radius > 0.0f) || !(s.probe_radius > 0.0f) || !(s.gravity_accel > 0.0f))
        return "eye_height, collision_radius, probe_radius and gravity_accel of a shape must be positive";
    if (s.ground_clearance < 0.0f || s.jump_speed < 0.0f) return "ground_clearance and jump_speed of a shape must not be negative";
    if (s.eye_height > YCGE_BODY_SHAPE_MAX_SIZE || s.collision_radius > YCGE_BODY_SHAPE_MAX_SIZE)
        return "eye_height or collision_radius of a shape above YCGE_BODY_SHAPE_MAX_SIZE (64)";
    return nullptr;
}
YCGE_HD const char *cam_status_text(int status)
{
    return status == ST_CAP_HORIZONTAL ? "a horizontal move reached the cap of YCGE_CAMERA_MAX_MICRO_STEPS (1024) micro-steps"
         : status == ST_CAP_VERTICAL   ? "a vertical move reached the cap of YCGE_CAMERA_MAX_MICRO_STEPS (1024) micro-steps"
                                       : "the camera position stopped being finite";
}

// the whole tick on the host: hit(rays, n, hits) answers a window (0 = fine, else the tick stops with that code); window = 1: serial order
template <class HitFn> int cam_run_host(Tick &t, HitFn hit, int window)
{
    Ray rays[kMaxWindow];
    Hit hits[kMaxWindow];
    while (cam_running(t)) {
        const int n = cam_take(t, window);
        for (int k = 0; k < n; k++) cam_ray(t, t.gi + k, rays[k]);
        const int e = hit(rays, n, hits);
        if (e != 0) return e;
        cam_commit(t, hits, n);
    }
    return 0;
}

// ---- the records of k_camera_tick (csrc/ycge_camera.hip; staged by csrc/ycge_camera.cpp): what one tick reads, and the one record it stores
struct TickIn {
    ycge_camera_body body;
    ycge_camera_world world;
    float dt_ms;
    int32_t n_moves, run_update;
    uint32_t pad[4];
    ycge_camera_move moves[YCGE_CAMERA_MAX_MOVES];
};
struct TickOut {
    ycge_camera_body body;
    ycge_camera_tick_info info;
    int32_t bad_move;
    int32_t status;               // ST_*, stored last; the host fills the record with 0xff before the launch
};
// ---- the records of k_bodies_tick: one header, an input record a body, the moves of all bodies as ONE array (body i's are
// moves[first_move .. first_move + n_moves)), and a TickOut a body
struct BodiesHeader {
    ycge_camera_world world;
    float dt_ms;
    int32_t run_update, n, n_moves_total;
    uint32_t pad;
};
struct BodyIn {
    ycge_camera_body body;
    ycge_body_shape shape;
    int32_t first_move, n_moves;
    uint32_t pad[2];
};
static_assert(sizeof(ycge_body_shape) == 24 && sizeof(ycge_body_result) == 8 && sizeof(BodiesHeader) == 32 && sizeof(BodyIn) == 80, "k_bodies_tick's records");
static_assert(sizeof(ycge_camera_body) == 40 && sizeof(ycge_camera_world) == 12 && sizeof(ycge_camera_move) == 16 && sizeof(ycge_camera_tick_info) == 48, "ycge.h");
static_assert(sizeof(TickIn) == 80 + 16 * YCGE_CAMERA_MAX_MOVES && sizeof(TickOut) == 96, "k_camera_tick's records");

} // namespace ycge_cam
