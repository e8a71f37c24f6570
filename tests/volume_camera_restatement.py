"""VolumeScene's camera physics restated from the reference in numpy scalars - the yardstick of ycge_volume_camera_tick and of the
stepper's host hook (tests/test_volume_camera_cpu.py, tests/test_gpu_volume_camera.py).

Written from Scenes/VolumeScenes.cs, method by method, in the reference's serial order and in its types: `CameraPos` is a Vec3 of three
binary32 (Vec3.cs:13-26: the (double, double, double) constructor rounds each component), `float` locals and constants are np.float32,
`double` locals np.float64; float op float stays float, float op double widens (C#'s rules).  Every constant is wrapped explicitly so that
no Python float takes part in an operation.  Scene.Hit is a callable

    hit(o, d, tmin, tmax) -> None | (t, (nx, ny, nz))          o, d: three np.float32 each; d as handed to `new Ray(o, d)`

which normalises d itself (Ray.cs:8-12), as the oracle's orc_scene_hit and the library's queries do.

An optional `observer(name, left, right, outcome)` is told of every comparison the physics decide by (tests/camera_seams.py names
them); it sees values only, the default is none, and nothing the restatement returns depends on it.

What is NOT the reference's: the observer, the counters (the same the library reports in ycge_camera_tick_info), the list of moves in place of
HandleInput's key decoding (a move is what one HandleInput call does to the body, :165-213), and `max_micro`, the most micro-steps one
move took - the reference's AttemptMoveHorizontal has no bound (:275 adds the slide's residual back), the library caps it.
"""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64

# VolumeScenes.cs:20-39
EyeHeight = F(1.7)
GravityAccel = F(9.81)
MaxProbeHeight = F(4096.0)
GroundClearance = F(0.10)
JumpSpeed = F(4.8)
LocalProbeDepthMin = F(3.0)
LocalProbeStart = F(0.6)
ProbeRadius = F(0.35)
ExtraFallMargin = F(1.0)
StepUpGuardEpsilon = F(0.05)
ShiftSpeedMult = F(30.0)
ShiftHoldGraceSeconds = F(0.15)
CollisionRadius = F(0.65)

MOVE_HORIZONTAL, MOVE_VERTICAL, MOVE_JUMP, MOVE_SHIFT = 0, 1, 2, 3
COUNTERS = ("rays_committed", "micro_steps", "blocked_steps", "slides", "push_outs", "embedded_resolutions", "ground_snaps", "auto_placements",
            "fail_safes")


def vec3(x, y, z):
    """new Vec3(double, double, double), Vec3.cs:21-26 (exact for float arguments)"""
    return [F(x), F(y), F(z)]


def normalized(v):
    """Vec3.Normalized, Vec3.cs:98-107"""
    len_sq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    if len_sq <= F(0.0):
        return list(v)
    inv = F(1.0) / np.sqrt(len_sq)
    return [v[0] * inv, v[1] * inv, v[2] * inv]


def dmax(a, b):
    """Math.Max(double, double): a NaN wins, +0 is greater than -0"""
    a, b = D(a), D(b)
    if np.isnan(a): return a
    if np.isnan(b): return b
    if a == b: return b if np.signbit(a) else a
    return a if a > b else b


def dmin(a, b):
    """Math.Min(double, double): a NaN wins, -0 is less than +0"""
    a, b = D(a), D(b)
    if np.isnan(a): return a
    if np.isnan(b): return b
    if a == b: return a if np.signbit(a) else b
    return a if a < b else b


class VolumeCamera:
    """the fields VolumeScene keeps between ticks (:16-43) and WorldConfig's three values its physics read"""

    def __init__(self, hit, pos, world_height, water_level, voxel_size_y, auto_placed=False, observer=None):
        self.hit = hit
        self.observer = observer
        self.CameraPos = vec3(*pos)
        self.autoPlaced = bool(auto_placed)
        self.verticalVelocity = F(0.0)
        self.shiftHoldTimer = F(0.0)
        self.repelVel = vec3(0.0, 0.0, 0.0)
        self.isGrounded = False
        self.WorldHeight, self.WaterLevel, self.VoxelSizeY = F(world_height), F(water_level), F(voxel_size_y)
        self.counters = dict.fromkeys(COUNTERS, 0)
        self.max_micro = 0

    # ------------------------------------------------------------------------------------------------ Scene.Hit
    def Hit(self, origin, d, tmin, tmax, group="ray"):
        self.counters["rays_committed"] += 1
        rec = self.hit([F(origin[0]), F(origin[1]), F(origin[2])], [F(d[0]), F(d[1]), F(d[2])], F(tmin), F(tmax))
        if self.observer is not None:                            # "hit:<group>": rec.T (None: no hit) against the ray's tMax
            self.observer("hit:" + group, None if rec is None else F(rec[0]), F(tmax), rec is not None)
        return rec

    def cmp(self, name, left, right, outcome):
        """a comparison's outcome, passed through; the observer is told its two sides"""
        if self.observer is not None:
            self.observer(name, left, right, bool(outcome))
        return outcome

    # ------------------------------------------------------------------------------------------------ one tick
    def tick(self, moves, delta_time_ms, run_update=True):
        """moves: (kind, shift, a, b) in the order received, then Update when run_update"""
        self.counters = dict.fromkeys(COUNTERS, 0)
        for kind, shift, a, b in moves:
            if kind == MOVE_SHIFT:
                self.shiftHoldTimer = ShiftHoldGraceSeconds                                   # :177
            elif kind == MOVE_JUMP:
                if not shift and self.cmp("jump_grounded", self.isGrounded, True, self.isGrounded):  # :208-212
                    self.verticalVelocity = JumpSpeed
                    self.isGrounded = False
            elif kind == MOVE_HORIZONTAL:
                self.AttemptMoveHorizontal(vec3(F(a), 0.0, F(b)))                               # :198-201
            elif kind == MOVE_VERTICAL:
                self.AttemptMoveVertical(D(F(a)))                                               # :204-205
            else:
                raise ValueError(kind)
        if run_update:
            self.Update(F(delta_time_ms))
        return dict(self.counters)

    # ------------------------------------------------------------------------------------------------ Update, :51-159
    def Update(self, deltaTimeMS):
        dt = F(deltaTimeMS)
        if self.cmp("dt_negative", dt, F(0.0), dt < F(0.0)): dt = F(0.0)
        dt = dt * F(0.001)
        self.ResolveIfEmbedded()                                                                # :72
        P = self.CameraPos
        if not self.autoPlaced:                                                                 # :75-86
            self.cmp("probe_top", self.WorldHeight + F(16.0), MaxProbeHeight, self.WorldHeight + F(16.0) < MaxProbeHeight)
            probeTop = D(min(self.WorldHeight + F(16.0), MaxProbeHeight))
            ok, g0 = self.TrySampleGroundYFan(D(P[0]), D(P[2]), probeTop, probeTop + D(F(8.0)))
            if self.cmp("auto_ground", ok, True, ok):
                self.CameraPos = vec3(P[0], g0 + D(EyeHeight) + D(GroundClearance), P[2])
            else:
                self.CameraPos = vec3(P[0], self.WaterLevel + EyeHeight + F(4.0), P[2])
            self.verticalVelocity = F(0.0)
            self.autoPlaced = True
            self.counters["auto_placements"] += 1
            return
        if self.cmp("timer_running", self.shiftHoldTimer, F(0.0), self.shiftHoldTimer > F(0.0)):       # :89-92
            self.cmp("timer_left", self.shiftHoldTimer - dt, F(0.0), self.shiftHoldTimer - dt > F(0.0))
            self.shiftHoldTimer = max(F(0.0), self.shiftHoldTimer - dt)
        shiftFlyActive = self.shiftHoldTimer > F(0.0)
        if not shiftFlyActive:                                                                  # :95-142
            self.verticalVelocity = self.verticalVelocity - GravityAccel * dt
            newY = D(P[1] + self.verticalVelocity * dt)
            fallDist = dmax(D(0.0), D(P[1]) - newY)
            probeDepth = dmax(D(LocalProbeDepthMin), fallDist + D(ExtraFallMargin))
            localProbeStartY = D(P[1] + LocalProbeStart)
            hasGround, ground = self.TrySampleGroundYFan(D(P[0]), D(P[2]), localProbeStartY, probeDepth + D(LocalProbeStart))
            self.isGrounded = False
            if hasGround:
                floorY = ground + D(EyeHeight) + D(GroundClearance)
                floorIsAboveHead = self.cmp("floor_above_head", floorY, D(P[1] + StepUpGuardEpsilon), floorY > D(P[1] + StepUpGuardEpsilon))
                if self.cmp("snap", newY, floorY, newY <= floorY) and not floorIsAboveHead:
                    newY = floorY
                    self.verticalVelocity = F(0.0)
                    self.isGrounded = True
                    self.counters["ground_snaps"] += 1
                else:
                    self.isGrounded = (not floorIsAboveHead) and bool(self.cmp("grounded", D(P[1]) - floorY, D(StepUpGuardEpsilon),
                                                                               (D(P[1]) - floorY) <= D(StepUpGuardEpsilon)))
            self.CameraPos = P = vec3(P[0], newY, P[2])
            corrStartY = D(P[1] + LocalProbeStart)
            corrDepth = D(LocalProbeStart) + D(1.5)
            ok, g2 = self.TrySampleGroundYFan(D(P[0]), D(P[2]), corrStartY, corrDepth)
            if ok:
                f2 = g2 + D(EyeHeight) + D(GroundClearance)
                if (self.cmp("corr_accept", f2, D(P[1] + StepUpGuardEpsilon), f2 <= D(P[1] + StepUpGuardEpsilon))
                        and self.cmp("hover", D(P[1]) - f2, D(0.5), (D(P[1]) - f2) <= D(0.5))):
                    self.CameraPos = P = vec3(P[0], f2, P[2])
                    self.verticalVelocity = F(0.0)
                    self.isGrounded = True
                    self.counters["ground_snaps"] += 1
        else:
            self.verticalVelocity = F(0.0)                                                      # :146
        self.ApplyWallRepulsion(dt)                                                             # :150
        P = self.CameraPos
        if self.cmp("fail_safe", D(P[1]), D(-10.0), D(P[1]) < D(-10.0)):                        # :153-158
            self.CameraPos = vec3(P[0], 200.0, P[2])
            self.verticalVelocity = F(0.0)
            self.repelVel = vec3(0.0, 0.0, 0.0)
            self.counters["fail_safes"] += 1

    # ------------------------------------------------------------------------------------------------ AttemptMoveHorizontal, :219-279
    def AttemptMoveHorizontal(self, delta):
        maxStep = dmax(D(0.1), D(CollisionRadius) * D(0.35))
        remaining = np.sqrt(D(delta[0] * delta[0] + delta[2] * delta[2]))
        if self.cmp("h_cutoff", remaining, D(1e-6), remaining <= D(1e-6)): return
        dir_ = vec3(D(delta[0]) / remaining, 0.0, D(delta[2]) / remaining)
        perp = vec3(-dir_[2], 0.0, dir_[0])
        micro = 0
        while self.cmp("h_remaining", remaining, D(1e-6), remaining > D(1e-6)):
            micro += 1
            self.max_micro = max(self.max_micro, micro)
            self.counters["micro_steps"] += 1
            self.cmp("h_step", remaining, maxStep, remaining < maxStep)
            step = dmin(remaining, maxStep)
            ref = dict(best=step, hadNormal=False, blockNormal=vec3(0.0, 0.0, 0.0))
            P = self.CameraPos
            eyeY = D(P[1])
            torsoY = D(P[1]) - (D(EyeHeight) * D(0.5))
            r = D(CollisionRadius)
            for o in (D(0.0), r, -r):
                offVec = vec3(D(perp[0]) * o, 0.0, D(perp[2]) * o)
                self.LimitStepByRay(vec3(P[0] + offVec[0], eyeY, P[2] + offVec[2]), dir_, ref)
                self.LimitStepByRay(vec3(P[0] + offVec[0], torsoY, P[2] + offVec[2]), dir_, ref)
            best = ref["best"]
            if self.cmp("caps_blocked", best, D(1e-5), best <= D(1e-5)):
                self.counters["blocked_steps"] += 1
                break
            self.CameraPos = vec3(D(P[0]) + D(dir_[0]) * best, P[1], D(P[2]) + D(dir_[2]) * best)
            remaining = remaining - best
            residual = step - best
            if self.cmp("residual", residual, D(1e-6), residual > D(1e-6)) and ref["hadNormal"]:
                slide = self.ProjectOntoPlaneXZ(dir_, ref["blockNormal"])
                length = np.sqrt(slide[0] * slide[0] + slide[2] * slide[2])
                if self.cmp("slide_length", length, F(1e-6), length > F(1e-6)):
                    dir_ = vec3(slide[0] / length, 0.0, slide[2] / length)
                    remaining = remaining + residual
                    self.counters["slides"] += 1

    def LimitStepByRay(self, origin, dir_, ref):                                               # :283-298
        tmax = F(ref["best"] + D(1e-3))
        rec = self.Hit(origin, dir_, F(0.001), tmax, "caps")
        if rec is not None:
            cand = dmax(D(0.0), D(F(rec[0])) - D(0.01))
            if self.cmp("caps_cand", cand, ref["best"], cand < ref["best"]):
                ref["best"] = cand
                ref["hadNormal"] = True
                ref["blockNormal"] = vec3(*rec[1])

    # ------------------------------------------------------------------------------------------------ AttemptMoveVertical, :300-325
    def AttemptMoveVertical(self, dy):
        dy = D(dy)
        if self.cmp("v_cutoff", abs(dy), D(1e-6), abs(dy) <= D(1e-6)): return
        remaining = D(abs(dy))
        stepSign = D(np.sign(dy))
        maxStep = dmax(D(0.1), D(EyeHeight) * D(0.25))
        micro = 0
        while self.cmp("v_remaining", remaining, D(1e-6), remaining > D(1e-6)):
            micro += 1
            self.max_micro = max(self.max_micro, micro)
            self.counters["micro_steps"] += 1
            self.cmp("v_step", remaining, maxStep, remaining < maxStep)
            step = dmin(remaining, maxStep)
            P = self.CameraPos
            rec = self.Hit(vec3(P[0], P[1], P[2]), vec3(0.0, stepSign, 0.0), F(0.001), F(step + D(1e-3)), "vert")
            if rec is not None:
                cand = dmax(D(0.0), D(F(rec[0])) - D(0.01))
                if self.cmp("vert_blocked", cand, D(1e-5), cand <= D(1e-5)):
                    self.counters["blocked_steps"] += 1
                    break
                self.CameraPos = vec3(P[0], D(P[1]) + cand * stepSign, P[2])
            else:
                self.CameraPos = vec3(P[0], D(P[1]) + step * stepSign, P[2])
            remaining = remaining - step

    # ------------------------------------------------------------------------------------------------ ResolveIfEmbedded, :328-414
    def ResolveIfEmbedded(self):
        if not self.IsLikelyEmbedded(): return
        dirs = [vec3(1, 0, 0), vec3(-1, 0, 0), vec3(0, 0, 1), vec3(0, 0, -1), vec3(0, 1, 0), vec3(0, -1, 0)]
        P = self.CameraPos
        eyeY = D(P[1])
        torsoY = D(P[1]) - (D(EyeHeight) * D(0.5))
        searchR = F(dmax(D(CollisionRadius) * D(4.0), D(self.VoxelSizeY) * D(4.0)))
        found, bestT, bestDir = False, D(np.inf), vec3(0.0, 1.0, 0.0)
        for d in dirs:
            for y in (eyeY, torsoY):
                rec = self.Hit(vec3(P[0], y, P[2]), d, F(0.0), searchR, "exit")                 # RayDist, :407-414
                if rec is not None and self.cmp("exit_t", D(F(rec[0])), bestT, D(F(rec[0])) < bestT):
                    bestT, bestDir, found = D(F(rec[0])), d, True
        if found and bestT < D(np.inf):
            eps = dmax(D(0.02), D(self.VoxelSizeY) * D(0.02))
            self.CameraPos = vec3(D(P[0]) + D(bestDir[0]) * (bestT + eps), D(P[1]) + D(bestDir[1]) * (bestT + eps), D(P[2]) + D(bestDir[2]) * (bestT + eps))
            self.counters["embedded_resolutions"] += 1
            self.ApplyWallRepulsion(F(0.0))
            self.ApplyWallRepulsion(F(0.0))

    def IsLikelyEmbedded(self):                                                                 # :382-387 (|| short-circuits)
        P = self.CameraPos
        eyeY = D(P[1])
        torsoY = D(P[1]) - (D(EyeHeight) * D(0.5))
        return (self.cmp("embedded_eye", None, None, self.IsLikelyEmbeddedAtY(eyeY))
                or self.cmp("embedded_torso", None, None, self.IsLikelyEmbeddedAtY(torsoY)))

    def IsLikelyEmbeddedAtY(self, y):                                                           # :389-398 (four statements, all evaluated)
        probe = F(dmax(D(0.05), D(CollisionRadius) * D(0.25)))
        P = self.CameraPos
        o = vec3(P[0], y, P[2])
        xPos = self.Hit(o, vec3(1, 0, 0), F(0.0), probe, "embed") is not None                            # RayHitWithin, :400-405
        xNeg = self.Hit(o, vec3(-1, 0, 0), F(0.0), probe, "embed") is not None
        zPos = self.Hit(o, vec3(0, 0, 1), F(0.0), probe, "embed") is not None
        zNeg = self.Hit(o, vec3(0, 0, -1), F(0.0), probe, "embed") is not None
        return (xPos and xNeg) and (zPos and zNeg)

    # ------------------------------------------------------------------------------------------------ ApplyWallRepulsion, :418-464
    def ApplyWallRepulsion(self, dt):
        eps = F(0.01)
        dirs = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]
        eyeY = D(self.CameraPos[1])
        torsoY = D(self.CameraPos[1]) - (D(EyeHeight) * D(0.5))
        for _ in range(2):
            for dx, dz in dirs:
                dx, dz = D(dx), D(dz)
                length = np.sqrt(dx * dx + dz * dz)
                dirXZ = vec3(dx / length, 0.0, dz / length)
                self.ResolvePenetrationAt(vec3(self.CameraPos[0], eyeY, self.CameraPos[2]), dirXZ, eps)
                self.ResolvePenetrationAt(vec3(self.CameraPos[0], torsoY, self.CameraPos[2]), dirXZ, eps)

    def ResolvePenetrationAt(self, origin, dirXZ, eps):
        rec = self.Hit(origin, dirXZ, F(0.001), CollisionRadius, "push")
        if rec is not None:
            pen = CollisionRadius - F(rec[0])
            if self.cmp("pen", pen, F(0.0), pen > F(0.0)):
                n = vec3(*rec[1])
                nXZ = vec3(n[0], 0.0, n[2])
                nl = np.sqrt(nXZ[0] * nXZ[0] + nXZ[2] * nXZ[2])
                if self.cmp("push_normal", nl, F(1e-6), nl > F(1e-6)):
                    nXZ = vec3(nXZ[0] / nl, 0.0, nXZ[2] / nl)
                    push = pen + eps
                    P = self.CameraPos
                    self.CameraPos = vec3(P[0] + nXZ[0] * push, P[1], P[2] + nXZ[2] * push)
                    self.counters["push_outs"] += 1

    @staticmethod
    def ProjectOntoPlaneXZ(v, n):                                                               # :466-474
        nXZ = vec3(n[0], 0.0, n[2])
        nl = np.sqrt(nXZ[0] * nXZ[0] + nXZ[2] * nXZ[2])
        if nl <= F(1e-6): return vec3(0.0, 0.0, 0.0)
        nXZ = vec3(nXZ[0] / nl, 0.0, nXZ[2] / nl)
        dot = F(v[0] * nXZ[0] + v[2] * nXZ[2])
        return vec3(v[0] - dot * nXZ[0], 0.0, v[2] - dot * nXZ[2])

    # ------------------------------------------------------------------------------------------------ ground fan, :478-530
    def TrySampleGroundYFan(self, x, z, startY, maxDistance):
        groundY = D(-np.inf)
        anyHit = anyAcceptable = False
        bestAcceptable = D(-np.inf)
        r = D(ProbeRadius)
        for ox, oz in ((D(0.0), D(0.0)), (r, D(0.0)), (-r, D(0.0)), (D(0.0), r), (D(0.0), -r)):
            ok, y = self.TrySampleGroundY(x + ox, z + oz, startY, maxDistance)
            if ok:
                anyHit = True
                floorCandidate = y + D(EyeHeight) + D(GroundClearance)
                guard = D(self.CameraPos[1] + StepUpGuardEpsilon)
                if self.cmp("fan_accept", floorCandidate, guard, floorCandidate <= guard):
                    if not anyAcceptable or self.cmp("fan_best", y, bestAcceptable, y > bestAcceptable): bestAcceptable = y
                    anyAcceptable = True
                if not anyAcceptable and (np.isneginf(groundY) or self.cmp("fan_ground", y, groundY, y > groundY)): groundY = y
        if anyAcceptable:
            return True, bestAcceptable
        return bool(anyHit and not np.isneginf(groundY)), groundY

    def TrySampleGroundY(self, x, z, startY, maxDistance):
        origin, d = vec3(x, startY, z), vec3(0.0, -1.0, 0.0)
        rec = self.Hit(origin, d, F(0.00001), F(maxDistance), "fan")
        if rec is None: return False, D(0.0)
        nd = normalized(d)
        t = F(rec[0])
        p = [origin[0] + nd[0] * t, origin[1] + nd[1] * t, origin[2] + nd[2] * t]             # Ray.At, Ray.cs:14-17
        return True, D(p[1])

    # ------------------------------------------------------------------------------------------------ the body as the library lays it out
    def body(self):
        """(pos[3], vertical_velocity, shift_hold_timer, repel_vel[3]) as float32 and (auto_placed, is_grounded)"""
        f = np.array([*self.CameraPos, self.verticalVelocity, self.shiftHoldTimer, *self.repelVel], np.float32)
        return f, (int(self.autoPlaced), int(self.isGrounded))
